"""Records tests/golden/fmif_ref.npz: the reference's FM IF noise reduction (dsp/noise_reduction/fm_if.h, compiled unmodified against
oracle/shim) run over a handful of inputs.  Only the recorded DATA is committed; the harness below is this project's own and is compiled into
a temporary directory.

    python tests/golden/make_fmif_golden.py /path/to/SDRPlusPlus

The reference links whatever libfftw3f is installed; oracle/shim's fftw3.h has a forward transform only.  The harness therefore puts an
fftw3.h of its own first on the include path: a plain O(N^2) DFT of either sign, evaluated in double and rounded to float — the "exact DFT"
FMIF is defined against (include/sdrpp_gpu.h, sdrpp_vfo_set_fmnr).

Per case: input `x`, the schedule `ops` (rows of (kind, value): 0 = process `value` samples, 1 = setBins(value), 2 = reset), the initial bin
count `bins`, the output `y`, and from a second run that feeds the block one sample at a time (the harness checks that it gives the same
output, bit for bit): `idx` (the winning bin) and `top` (the two largest magnitudes) of every sample."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FFTW_H = r"""
// An exact DFT behind the four libfftw3f entry points fm_if.h uses: O(N^2), either sign, evaluated in double, rounded to float.
#pragma once
#include <math.h>
#include <stdlib.h>
typedef float fftwf_complex[2];
struct exact_dft_plan { int n, sign; fftwf_complex* in; fftwf_complex* out; };
typedef struct exact_dft_plan* fftwf_plan;
#define FFTW_FORWARD (-1)
#define FFTW_BACKWARD (+1)
#define FFTW_ESTIMATE (1U << 6)
static inline void* fftwf_malloc(size_t n) { void* p = NULL; if (posix_memalign(&p, 64, n ? n : 64)) { return NULL; } return p; }
static inline void fftwf_free(void* p) { free(p); }
static inline fftwf_plan fftwf_plan_dft_1d(int n, fftwf_complex* in, fftwf_complex* out, int sign, unsigned flags) {
    (void)flags;
    fftwf_plan p = (fftwf_plan)malloc(sizeof(struct exact_dft_plan));
    p->n = n; p->sign = sign; p->in = in; p->out = out;
    return p;
}
static inline void fftwf_execute(const fftwf_plan p) {
    const double tau = 6.283185307179586476925286766559;
    for (int k = 0; k < p->n; k++) {
        double re = 0.0, im = 0.0;
        for (int n = 0; n < p->n; n++) {
            const int m = (int)(((long long)k * n) % p->n);
            const double a = (double)p->sign * tau * (double)m / (double)p->n, c = cos(a), s = sin(a);
            re += (double)p->in[n][0] * c - (double)p->in[n][1] * s;
            im += (double)p->in[n][0] * s + (double)p->in[n][1] * c;
        }
        p->out[k][0] = (float)re;
        p->out[k][1] = (float)im;
    }
}
static inline void fftwf_destroy_plan(fftwf_plan p) { free(p); }
"""

HARNESS = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "dsp/noise_reduction/fm_if.h"
struct Probe : public dsp::noise_reduction::FMIF {
    // after process(1, ...): the spectrum and magnitudes of that sample's window are still in the block's buffers
    void look(unsigned* idx, float* top) {
        unsigned best = 0;
        for (int k = 1; k < _bins; k++) { if (ampBuf[k] > ampBuf[best]) { best = (unsigned)k; } }
        float second = -1.0f;
        for (int k = 0; k < _bins; k++) { if ((unsigned)k != best && ampBuf[k] > second) { second = ampBuf[k]; } }
        *idx = best;
        top[0] = ampBuf[best];
        top[1] = second;
    }
};
// argv: in.bin out.bin probe.bin bins op...      op: c<count> | b<bins> | r
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n), y((size_t)n), y1((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    std::vector<unsigned> idx((size_t)n);
    std::vector<float> top((size_t)2 * n);
    dsp::stream<dsp::complex_t> dummy;
    dsp::noise_reduction::FMIF blk;
    Probe one;
    blk.init(&dummy, atoi(argv[4]));
    one.init(&dummy, atoi(argv[4]));
    long pos = 0;
    for (int a = 5; a < argc; a++) {
        const int v = atoi(argv[a] + 1);
        if (argv[a][0] == 'b') { blk.setBins(v); one.setBins(v); }
        else if (argv[a][0] == 'r') { blk.reset(); one.reset(); }
        else {
            blk.process(v, x.data() + pos, y.data() + pos);
            for (int i = 0; i < v; i++) {
                one.process(1, x.data() + pos + i, y1.data() + pos + i);
                one.look(&idx[(size_t)(pos + i)], &top[(size_t)2 * (pos + i)]);
            }
            pos += v;
        }
    }
    if (pos != n) { return 3; }
    if (memcmp(y.data(), y1.data(), (size_t)n * sizeof(dsp::complex_t)) != 0) { return 4; }
    f = fopen(argv[2], "wb");
    fwrite(y.data(), sizeof(dsp::complex_t), (size_t)n, f);
    fclose(f);
    f = fopen(argv[3], "wb");
    fwrite(idx.data(), sizeof(unsigned), (size_t)n, f);
    fwrite(top.data(), sizeof(float), (size_t)2 * n, f);
    fclose(f);
    return 0;
}
"""


def signal(n, seed, fade, rate):
    """FM carrier of amplitude 0.05 (2.5 kHz deviation, 1 kHz tone, 312 Hz off centre) + noise sigma 0.004 (+ a silent stretch and a 60 dB fade)"""
    r = np.random.default_rng(seed)
    t = np.arange(n) / rate
    x = 0.05 * np.exp(1j * (2 * np.pi * 312.0 * t + 2.5 * np.sin(2 * np.pi * 1000.0 * t)))
    x = x + 0.004 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    if fade:
        g = np.ones(n)
        g[n // 4:n // 4 + n // 8] = 0.0  # silence: exact-zero windows, every bin equal — bin 0 wins, the output is 0
        g[n // 2:] = 10.0 ** (-3.0 * np.arange(n - n // 2) / (n - n // 2))
        x = x * g
    return x.astype(np.complex64)


def blocks(n, size):
    return [(0, size)] * (n // size) + ([(0, n % size)] if n % size else [])


CASES = [
    # name, n, seed, fade, rate, bins, ops
    ("apt9", 1200, 1, False, 24000.0, 9, blocks(1200, 120)),
    ("voice15", 1200, 2, False, 24000.0, 15, blocks(1200, 120)),
    ("narrow31", 1200, 3, False, 24000.0, 31, blocks(1200, 120)),
    ("broadcast32", 1200, 4, False, 250000.0, 32, blocks(1200, 250)),
    ("apt9_fade", 960, 5, True, 24000.0, 9, blocks(960, 120)),
    ("voice15_fade", 960, 6, True, 24000.0, 15, blocks(960, 7) ),
    ("narrow31_fade", 960, 7, True, 24000.0, 31, blocks(960, 120)),
    ("broadcast32_fade", 960, 8, True, 250000.0, 32, blocks(960, 250)),
    ("setbins_mid", 900, 9, False, 24000.0, 15, blocks(360, 120) + [(1, 31)] + blocks(300, 100) + [(1, 32)] + blocks(240, 120)),
    ("reset_mid", 900, 10, False, 24000.0, 31, blocks(450, 90) + [(2, 0)] + blocks(450, 150)),
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
        with open(os.path.join(tmp, "fftw3.h"), "w") as f:
            f.write(FFTW_H)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + tmp, "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "core", "src"), "-o", exe, src,
                        "-lpthread"], check=True)
        names = []
        for name, n, seed, fade, rate, bins, ops in CASES:
            assert sum(v for k, v in ops if k == 0) == n, name
            x = signal(n, seed, fade, rate)
            fin, fout, fpr = (os.path.join(tmp, q) for q in ("in.bin", "out.bin", "probe.bin"))
            x.tofile(fin)
            toks = [("c%d" % v) if k == 0 else (("b%d" % v) if k == 1 else "r") for k, v in ops]
            subprocess.run([exe, fin, fout, fpr, str(bins)] + toks, check=True)
            raw = np.fromfile(fpr, np.uint8)
            out[name + "_x"] = x
            out[name + "_ops"] = np.asarray(ops, np.int32)
            out[name + "_bins"] = np.asarray(bins, np.int32)
            out[name + "_y"] = np.fromfile(fout, np.complex64)
            out[name + "_idx"] = raw[:4 * n].view(np.uint32).astype(np.uint8)
            out[name + "_top"] = raw[4 * n:].view(np.float32).reshape(n, 2)
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "fmif_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
