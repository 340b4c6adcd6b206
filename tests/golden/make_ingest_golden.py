"""Records tests/golden/ingest_ref.npz: what the reference's SDR++-server client makes of the frames it receives —
dsp::compression::SampleStreamDecompressor::process (core/src/dsp/compression/sample_stream_decompressor.h), compiled unmodified against oracle/shim —
over a handful of frames.  Only the recorded DATA is committed; the harness below is this project's own and is compiled into a temporary directory.

    python tests/golden/make_ingest_golden.py /path/to/SDRPlusPlus

Per frame `name`: the frame's bytes (`<name>_frame`, uint8), the count process() returned (`<name>_count`) and the floats it wrote (`<name>_out`,
[count, 2]).  A frame is [u16 0][u16 type][f32 scaler][data]; PCMType: 0 I8, 1 I16, 2 F32."""
import os
import struct
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
#include "dsp/compression/sample_stream_decompressor.h"
// argv: frame.bin out.bin -> prints the returned count
int main(int argc, char** argv) {
    if (argc != 3) { return 1; }
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::vector<uint8_t> in((size_t)n + 16);
    if (fread(in.data(), 1, (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    std::vector<dsp::complex_t> out((size_t)n + 16);
    dsp::compression::SampleStreamDecompressor dec;
    const int count = dec.process((int)n, in.data(), out.data());
    f = fopen(argv[2], "wb");
    fwrite(out.data(), sizeof(dsp::complex_t), (size_t)count, f);
    fclose(f);
    printf("%d\n", count);
    return 0;
}
"""

I8, I16, F32 = 0, 1, 2
CASES = [
    # name, type, scaler, samples the data holds, spare bytes behind the last whole sample
    ("i8_s1_n1031", I8, 1.0, 1031, 0),
    ("i8_s037_n7", I8, 0.37, 7, 0),
    ("i8_s33e4_n1", I8, 3.3e-4, 1, 0),
    ("i8_s33e4_n1031", I8, 3.3e-4, 1031, 1),
    ("i16_s1_n7", I16, 1.0, 7, 0),
    ("i16_s037_n1031", I16, 0.37, 1031, 0),
    ("i16_s33e4_n1", I16, 3.3e-4, 1, 0),
    ("i16_s1_n1_spare", I16, 1.0, 1, 3),
    ("f32_n7", F32, 1.0, 7, 0),
    ("f32_n1031", F32, 0.37, 1031, 0),
    ("unknown_type", 3, 1.0, 7, 0),
    ("header_only", I16, 1.0, 0, 0),
    ("no_whole_sample", I8, 1.0, 0, 1),
]


def frame_bytes(r, typ, scaler, n, spare):
    if typ == I8:
        d = r.integers(-128, 128, 2 * n, dtype=np.int64).astype(np.int8)
        if n >= 2:
            d[:4] = [-128, 127, 0, -1]
    elif typ == I16:
        d = r.integers(-32768, 32768, 2 * n, dtype=np.int64).astype(np.int16)
        if n >= 2:
            d[:4] = [-32768, 32767, 0, -1]
    elif typ == F32:
        d = r.standard_normal(2 * n).astype(np.float32)
    else:
        d = r.integers(0, 256, 4 * n, dtype=np.int64).astype(np.uint8)
    return struct.pack("<HHf", 0, typ, scaler) + d.tobytes() + bytes(r.integers(0, 256, spare, dtype=np.int64).astype(np.uint8))


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
        for k, (name, typ, scaler, n, spare) in enumerate(CASES):
            fr = frame_bytes(np.random.default_rng(100 + k), typ, scaler, n, spare)
            pin, pout = os.path.join(tmp, "frame.bin"), os.path.join(tmp, "out.bin")
            with open(pin, "wb") as f:
                f.write(fr)
            res = subprocess.run([exe, pin, pout], check=True, capture_output=True, text=True)
            count = int(res.stdout.strip())
            out[name + "_frame"] = np.frombuffer(fr, np.uint8).copy()
            out[name + "_count"] = np.asarray([count], np.int32)
            out[name + "_out"] = np.fromfile(pout, np.float32).reshape(-1, 2)
            assert len(out[name + "_out"]) == count, (name, count)
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "ingest_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
