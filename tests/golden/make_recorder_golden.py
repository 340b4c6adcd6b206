"""Records tests/golden/recorder_ref.npz: the blocks the reference's recorder puts behind a radio's audio stream — dsp/audio/volume.h,
dsp/convert/stereo_to_mono.h and dsp/bench/peak_level_meter.h, compiled unmodified against oracle/shim — run over a handful of inputs.  Only the
recorded DATA is committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_recorder_golden.py /path/to/SDRPlusPlus

Per case: stereo input `x` [n, 2], the slider value `vol`, the block cut `cut`, and: the volume's output `v`, the mono fold `m` of it, and the meter's level
after every block of the cut (`lvl` [blocks, 2]: the running maximum)."""
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
#include "dsp/audio/volume.h"
#include "dsp/convert/stereo_to_mono.h"
#include "dsp/bench/peak_level_meter.h"
// argv: in.bin v.bin m.bin lvl.bin volume cut...
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::stereo_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::stereo_t> x((size_t)n + 1), v((size_t)n + 1);
    std::vector<float> m((size_t)n + 1), lvl;
    if (n > 0 && fread(x.data(), sizeof(dsp::stereo_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    dsp::stream<dsp::stereo_t> dummy;
    dsp::audio::Volume vol;
    dsp::convert::StereoToMono s2m;
    dsp::bench::PeakLevelMeter<dsp::stereo_t> meter;
    vol.init(&dummy, atof(argv[5]), false);
    s2m.init(&dummy);
    meter.init(&dummy);
    long pos = 0;
    for (int a = 6; a < argc; a++) {
        const int c = atoi(argv[a]);
        vol.process(c, x.data() + pos, v.data() + pos);
        meter.process(c, v.data() + pos);
        s2m.process(c, v.data() + pos, m.data() + pos);
        const dsp::stereo_t l = meter.getLevel();
        lvl.push_back(l.l);
        lvl.push_back(l.r);
        pos += c;
    }
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb"); fwrite(v.data(), sizeof(dsp::stereo_t), (size_t)n, f); fclose(f);
    f = fopen(argv[3], "wb"); fwrite(m.data(), sizeof(float), (size_t)n, f); fclose(f);
    f = fopen(argv[4], "wb"); fwrite(lvl.data(), sizeof(float), lvl.size(), f); fclose(f);
    return 0;
}
"""

CASES = [
    # name, n, seed, amplitude, volume, block
    ("unity", 300, 1, 0.5, 1.0, 64),
    ("loud", 259, 2, 0.7, 8.0, 65),
    ("quiet", 130, 3, 0.3, 0.003, 63),
    ("odd_gain", 200, 4, 1.0, 0.77, 1),
    ("tiny", 64, 5, 1e-20, 0.31, 64),
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
        for name, n, seed, amp, vol, blk in CASES:
            r = np.random.default_rng(seed)
            x = (amp * r.standard_normal((n, 2))).astype(np.float32)
            x[n // 3] = 0.0
            x[n // 2, 1] = -x[n // 2, 0]  # the fold of a pair that cancels
            cut = [blk] * (n // blk) + ([n % blk] if n % blk else [])
            p = [os.path.join(tmp, k) for k in ("in.bin", "v.bin", "m.bin", "lvl.bin")]
            x.tofile(p[0])
            subprocess.run([exe] + p + [repr(vol)] + [str(c) for c in cut], check=True)
            out[name + "_x"] = x
            out[name + "_vol"] = np.asarray([vol], np.float64)
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_v"] = np.fromfile(p[1], np.float32).reshape(-1, 2)
            out[name + "_m"] = np.fromfile(p[2], np.float32)
            out[name + "_lvl"] = np.fromfile(p[3], np.float32).reshape(-1, 2)
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "recorder_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
