"""Records tests/golden/m17_ref.npz: the front of the reference's M17 decoder (decoder_modules/m17_decoder/src/m17dsp.h, compiled unmodified against oracle/shim
and two stand-in headers for the codec and FEC libraries it mentions) — dsp::demod::GFSK, M17Slice4FSK and M17FrameDemux — run over a handful of IF-rate inputs.
Only the recorded DATA is committed; the harness and the stand-in headers below are this project's own and are written to a temporary directory.

    python tests/golden/make_m17_golden.py /path/to/SDRPlusPlus

The harness drives GFSK::process block by block as M17Decoder::init sets it up (4800 baud, deviation 2400 Hz, 31 root-raised-cosine taps of alpha 0.5, omega gain
1e-6, mu gain 0.01, relative limit 0.01), hands each block's soft symbols to M17Slice4FSK and M17FrameDemux through the reference's own streams (run() called per
block; a polling reader thread per output stream takes what the demux swaps out and stamps it with a running number) and reaches private members by redefining the
access keywords.  M17FrameDemux::delay comes from new[] and is not initialised by the reference: the harness zeroes its first 16 entries after init.

Inputs are IF-rate I/Q (14.4 kS/s) stored as int16, value / 16384: 4FSK, root-raised-cosine shaped (alpha 0.5), outer deviation +-2400 Hz, 3 samples per symbol,
amplitude 0.5 — 96 dibits of +3 / -3 preamble, then sync word + 368 random bits five times (link setup, stream, stream, packet, stream), then a random tail —
beginning inside the preamble at full swing, shifted by 0, 1 or 2 samples, and noise.  Per case:
    <name>_x        int16 [n, 2]
    <name>_cut      the block schedule: samples per GFSK::process call
    <name>_reset    the blocks in front of which the whole chain was replaced by a fresh one
    <name>_soft     the soft symbols of all blocks, float32 [m];  <name>_counts  symbols per block
    <name>_dibits   uint8 [2 m]: what M17Slice4FSK swapped out
    <name>_pcl      after init: pcl.freq (omega), _minFreq, _maxFreq, _alpha (mu gain), _beta (omega gain), and the discriminator's _invDeviation — six float32
    <name>_taps     the 31 root-raised-cosine taps
    <name>_ftype    per frame: 0 link setup, 1 stream, 2 packet;  <name>_fblock  the block whose call delivered it;  <name>_fstream  the output stream that
                    carried its payload (0 linkSetupOut, 2 streamOut, 3 packetOut; types 1 and 2 also write lichOut, stream 1)
    <name>_frames   uint8 [frames, 368]: the frame in de-interleaved order — type 0 the 368 entries of linkSetupOut, types 1 / 2 the 96 of lichOut followed by
                    the first 272 of streamOut / packetOut (the reference swaps 368 there; the last 96 are whatever the buffer held)
    <name>_dev_max  the reference's own SPREAD as tests/golden/make_pager_golden.py records it: K = 8 further runs, every input sample multiplied by 1 +- 2^-24
                    with a random sign; per symbol the largest |soft - soft_0|, float32 [m];  <name>_dev_rms  the RMS of all those deviations
    <name>_settled  uint8 [m]: 0 for the 13 symbols a fresh chain starts while the filter's and the interpolator's delay lines (30 + 7 samples) still hold their
                    cleared content — partial sums that pass 0 by construction: the very first is 0 * taps + one sample times a tap of 1e-17 — 1 elsewhere
    <name>_startup_sign  int8 [m]: for those start-up symbols the sign all nine runs agree in (-1: negative, +1: not negative; the recorder asserts the agreement,
                    and that none is beyond the second threshold in one run and not in another), 0 for settled symbols: what their dibits rest on
and once: `scramble` uint8 [368], `interleave` uint16 [368], `sync` uint8 [3, 16] — the reference's three tables.
The recorder asserts: all nine runs of a case agree in the counts, in every dibit (the start-up ones included, and for those in sign and threshold side
explicitly) and in every frame; no settled soft value lies
within G of a decision level (0, +-high_cut), G = 10 x the case's largest per-symbol bar max(1e-5 * RMS, 4 * dev_max) (a case that fails gets another seed); the
aligned cases deliver five frames.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
RATE, BAUD, SPS = 14400.0, 4800.0, 3
K_SPREAD = 8
LEAD = 16     # preamble symbols generated in front of the 96 and cut off
STARTUP = 13  # symbols a fresh chain starts while its delay lines (30 + 7 samples) still hold their cleared content: ceil(37 / 3)
HIGH_CUT = (np.float32(1.0) + np.float32(1.0) / np.float32(3.0)) / np.float32(2.0)
SYNC = (0x55F7, 0xFF5D, 0x75FF)

CODEC2_H = r"""
#pragma once
// stand-in: the few names m17dsp.h mentions (the codec is not part of what is recorded)
struct CODEC2;
#define CODEC2_MODE_3200 0
inline CODEC2* codec2_create(int) { return nullptr; }
inline void codec2_destroy(CODEC2*) {}
inline int codec2_samples_per_frame(CODEC2*) { return 160; }
inline void codec2_decode(CODEC2*, short*, const unsigned char*) {}
"""
CORRECT_H = r"""
#pragma once
// stand-in: the few names m17dsp.h mentions (the Viterbi decoder is not part of what is recorded)
#include <stddef.h>
#include <stdint.h>
#include <sys/types.h>
typedef uint16_t correct_convolutional_polynomial_t;
struct correct_convolutional;
inline correct_convolutional* correct_convolutional_create(size_t, size_t, const correct_convolutional_polynomial_t*) { return nullptr; }
inline void correct_convolutional_destroy(correct_convolutional*) {}
inline ssize_t correct_convolutional_decode(correct_convolutional*, const uint8_t*, size_t, uint8_t*) { return 0; }
"""

HARNESS = r"""
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <volk/volk.h>
#define private public
#define protected public
#include "m17dsp.h"
#undef private
#undef protected
struct Rec { int seq, stream, block, n; std::vector<uint8_t> data; };
static std::mutex g_mtx;
static std::vector<Rec> g_recs;
static std::atomic<int> g_seq{ 0 }, g_block{ 0 };
struct Chain {
    dsp::stream<dsp::complex_t> dummy;
    dsp::demod::GFSK demod;
    dsp::stream<float> softS;
    dsp::M17Slice4FSK slice;
    dsp::M17FrameDemux demux;
    std::atomic<bool> quit{ false };
    std::thread readers[4];
    dsp::stream<uint8_t>* outs[4];
    Chain() {
        demod.init(&dummy, M17_BAUDRATE, 14400.0, M17_DEVIATION, 31, M17_RRC_ALPHA, 1e-6f, 0.01f, 0.01f);  // as M17Decoder::init calls it
        slice.init(&softS);
        demux.init(&slice.out);
        memset(demux.delay, 0, 16);
        outs[0] = &demux.linkSetupOut; outs[1] = &demux.lichOut; outs[2] = &demux.streamOut; outs[3] = &demux.packetOut;
        for (int s = 0; s < 4; s++) {
            readers[s] = std::thread([this, s] {
                dsp::stream<uint8_t>& st = *outs[s];
                while (!quit.load()) {
                    int n = -1;
                    {
                        std::lock_guard<std::mutex> lck(st.rdyMtx);
                        if (st.dataReady) { n = st.dataSize; }
                    }
                    if (n < 0) { continue; }
                    Rec r{ g_seq.fetch_add(1), s, g_block.load(), n, std::vector<uint8_t>(st.readBuf, st.readBuf + n) };
                    {
                        std::lock_guard<std::mutex> lck(g_mtx);
                        g_recs.push_back(std::move(r));
                    }
                    st.flush();
                }
            });
        }
    }
    void drain() {
        for (int s = 0; s < 4; s++) {
            for (;;) {
                std::lock_guard<std::mutex> lck(outs[s]->rdyMtx);
                if (!outs[s]->dataReady) { break; }
            }
        }
    }
    void retire() {  // (the object itself is left alone: the blocks' destructors would stop workers that never ran)
        drain();
        quit.store(true);
        for (auto& t : readers) { t.join(); }
    }
};
// argv: in.bin soft.bin counts.bin meta.bin taps.bin dibits.bin frames.bin tables.bin op...      op: c<count> | r (a fresh chain)
int main(int argc, char** argv) {
    FILE* f = fopen(argv[1], "rb");
    fseek(f, 0, SEEK_END);
    const long n = ftell(f) / (long)sizeof(dsp::complex_t);
    fseek(f, 0, SEEK_SET);
    std::vector<dsp::complex_t> x((size_t)n);
    if (fread(x.data(), sizeof(dsp::complex_t), (size_t)n, f) != (size_t)n) { return 2; }
    fclose(f);
    std::vector<float> soft((size_t)n + 64);
    std::vector<uint8_t> dibits;
    std::vector<int> counts;
    Chain* c = new Chain;
    float meta[6] = { c->demod.recov.pcl.freq, c->demod.recov.pcl._minFreq, c->demod.recov.pcl._maxFreq, c->demod.recov.pcl._alpha, c->demod.recov.pcl._beta, c->demod.demod._invDeviation };
    f = fopen(argv[4], "wb"); fwrite(meta, sizeof(float), 6, f); fclose(f);
    f = fopen(argv[5], "wb"); fwrite(c->demod.rrcTaps.taps, sizeof(float), c->demod.rrcTaps.size, f); fclose(f);
    f = fopen(argv[8], "wb");
    fwrite(M17_SCRAMBLER, 1, 368, f); fwrite(M17_INTERLEAVER, sizeof(uint16_t), 368, f);
    fwrite(M17_LSF_SYNC, 1, 16, f); fwrite(M17_STF_SYNC, 1, 16, f); fwrite(M17_PKF_SYNC, 1, 16, f);
    fclose(f);
    long pos = 0, ns = 0;
    int block = 0;
    for (int a = 9; a < argc; a++) {
        if (argv[a][0] == 'r') {
            c->retire();
            c = new Chain;
            continue;
        }
        const int v = atoi(argv[a] + 1);
        g_block.store(block);
        const int got = c->demod.process(v, x.data() + pos, soft.data() + ns);
        counts.push_back(got);
        if (got > 0) {  // (GFSK::run swaps only where symbols came out)
            memcpy(c->softS.writeBuf, soft.data() + ns, (size_t)got * sizeof(float));
            if (!c->softS.swap(got)) { return 4; }
            if (c->slice.run() != got) { return 5; }
            dibits.insert(dibits.end(), c->slice.out.readBuf, c->slice.out.readBuf + 2 * got);
            if (c->demux.run() != 2 * got) { return 6; }
            c->drain();
        }
        ns += got;
        pos += v;
        block++;
    }
    c->retire();
    if (pos != n) { return 3; }
    f = fopen(argv[2], "wb"); fwrite(soft.data(), sizeof(float), (size_t)ns, f); fclose(f);
    f = fopen(argv[3], "wb"); fwrite(counts.data(), sizeof(int), counts.size(), f); fclose(f);
    f = fopen(argv[6], "wb"); fwrite(dibits.data(), 1, dibits.size(), f); fclose(f);
    std::sort(g_recs.begin(), g_recs.end(), [](const Rec& a, const Rec& b) { return a.seq < b.seq; });
    f = fopen(argv[7], "wb");
    for (const Rec& r : g_recs) {
        const int head[3] = { r.stream, r.block, r.n };
        fwrite(head, sizeof(int), 3, f);
        fwrite(r.data.data(), 1, (size_t)r.n, f);
    }
    fclose(f);
    return 0;
}
"""


def rrc(count, beta, ts):
    """root-raised-cosine pulse, the textbook closed form, `ts` samples per symbol"""
    t = (np.arange(count) - (count - 1) / 2.0) / ts
    h = np.empty(count)
    for i, u in enumerate(t):
        if abs(u) < 1e-12:
            h[i] = 1.0 + beta * (4.0 / np.pi - 1.0)
        elif abs(abs(u) - 1.0 / (4.0 * beta)) < 1e-12:
            h[i] = beta / np.sqrt(2.0) * ((1.0 + 2.0 / np.pi) * np.sin(np.pi / (4.0 * beta)) + (1.0 - 2.0 / np.pi) * np.cos(np.pi / (4.0 * beta)))
        else:
            h[i] = (np.sin(np.pi * u * (1.0 - beta)) + 4.0 * beta * u * np.cos(np.pi * u * (1.0 + beta))) / (np.pi * u * (1.0 - (4.0 * beta * u) ** 2))
    return h


def signal(seed, delay, sigma, tail=144):
    """-> int16 [n, 2]"""
    r = np.random.default_rng(seed)
    level = {(0, 1): 1.0, (0, 0): 1.0 / 3.0, (1, 0): -1.0 / 3.0, (1, 1): -1.0}
    bits = []
    for t in (0, 1, 1, 2, 1):
        bits += [(SYNC[t] >> (15 - b)) & 1 for b in range(16)] + list(r.integers(0, 2, 368))
    bits += list(r.integers(0, 2, 2 * tail))
    sym = [1.0, -1.0] * (48 + LEAD // 2) + [level[(int(bits[i]), int(bits[i + 1]))] for i in range(0, len(bits), 2)]
    up = np.zeros(len(sym) * SPS + 60)
    up[30:30 + len(sym) * SPS:SPS] = sym
    h = rrc(61, 0.5, float(SPS))
    h = h / np.convolve(h, rrc(31, 0.5, float(SPS)) / float(SPS)).max()  # through the receiver's 31 taps (the same pulse / 3) a symbol comes out at its level
    f = np.convolve(up, h, mode="same") * 2400.0
    f = f[30 + LEAD * SPS - delay:]  # the stream begins inside the preamble, at full swing, with 96 dibits of it to come
    n = len(f)
    x = 0.5 * np.exp(1j * 2 * np.pi * np.cumsum(f) / RATE) + sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
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
    # name, seed, delay in samples, noise sigma per component, block sizes (cycled), blocks with a fresh chain in front of them, all five frames expected
    ("aligned_clean", 1, None, 0.0005, [600], [], True),
    ("aligned_noise", 2, None, 0.006, [600], [], True),
    ("aligned_noisy", 3, None, 0.02, [600], [], True),
    ("delay_a", 4, "a", 0.0005, [600], [], False),
    ("delay_b", 5, "b", 0.0005, [600], [], False),
    ("cuts", 6, None, 0.006, [997, 7, 1, 1250], [], True),
    ("reset", 7, None, 0.006, [600], [3], False),
]


def parse_frames(path):
    """the harness' records in the order the demux swapped them out -> (type, payload stream, block, uint8 [368]) per frame"""
    raw = open(path, "rb").read()
    recs, pos = [], 0
    while pos < len(raw):
        s, b, n = np.frombuffer(raw, np.int32, 3, pos)
        recs.append((int(s), int(b), np.frombuffer(raw, np.uint8, int(n), pos + 12).copy()))
        pos += 12 + int(n)
    per = {s: [r for r in recs if r[0] == s] for s in range(4)}
    frames, lich = [], list(per[1])
    for s, b, d in [r for r in recs if r[0] != 1]:
        if s == 0:
            assert len(d) == 368
            frames.append((0, 0, b, d))
        else:
            lb = lich.pop(0)
            assert lb[1] == b and len(lb[2]) == 96 and len(d) == 368, "a LICH record without its payload"
            frames.append((1 if s == 2 else 2, s, b, np.concatenate([lb[2], d[:272]])))
    assert not lich
    return frames


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "h.cpp"), os.path.join(tmp, "h")
        for name, text in (("h.cpp", HARNESS), ("codec2.h", CODEC2_H), ("correct.h", CORRECT_H)):
            with open(os.path.join(tmp, name), "w") as f:
                f.write(text)
        subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I" + tmp, "-I" + os.path.join(ROOT, "oracle", "shim"), "-I" + os.path.join(ref, "core", "src"),
                        "-I" + os.path.join(ref, "decoder_modules", "m17_decoder", "src"), "-o", exe, src, "-lpthread"], check=True)
        files = [os.path.join(tmp, k) for k in ("in.bin", "soft.bin", "counts.bin", "meta.bin", "taps.bin", "dibits.bin", "frames.bin", "tables.bin")]

        def run(x, toks):
            x.tofile(files[0])
            subprocess.run([exe] + files + toks, check=True)
            return (np.fromfile(files[1], np.float32), np.fromfile(files[2], np.int32), np.fromfile(files[5], np.uint8), parse_frames(files[6]))

        def n_frames(delay):
            q = signal(100, delay, 0.0005)
            x = (q.astype(np.float32) / np.float32(16384.0)).reshape(-1)
            return len(run(x, ["c%d" % s for s in schedule(len(q), [600])])[3])

        # the loop hardly re-times: of the three sample alignments one delivers every frame
        got = [n_frames(d) for d in range(3)]
        print("frames delivered at delays 0, 1, 2:", got)
        assert sorted(got)[-1] == 5
        aligned = int(np.argmax(got))
        others = [d for d in range(3) if d != aligned]
        delays = {None: aligned, "a": others[0], "b": others[1]}
        names = []
        for name, seed0, dkey, sigma, sizes, resets, all_five in CASES:
            for attempt in range(20):
                seed = seed0 + 100 * attempt
                q = signal(seed, delays[dkey], sigma)
                cut = schedule(len(q), sizes)
                x = (q.astype(np.float32) / np.float32(16384.0)).reshape(-1)  # interleaved re, im
                toks = []
                for b, s in enumerate(cut):
                    if b in resets:
                        toks.append("r")
                    toks.append("c%d" % s)
                soft, counts, dibits, frames = run(x, toks)
                r = np.random.default_rng(1000 + seed)
                dev = np.zeros((K_SPREAD, len(soft)), np.float64)
                runs = [soft]
                for k in range(K_SPREAD):
                    sgn = np.where(r.integers(0, 2, x.shape) == 1, 1.0, -1.0)
                    xk = (x.astype(np.float64) * (1.0 + sgn * 2.0 ** -24)).astype(np.float32)
                    sk, ck, dk, fk = run(xk, toks)
                    assert np.array_equal(ck, counts), "%s: run %d differs in its symbol counts" % (name, k)
                    assert np.array_equal(dk, dibits), "%s: run %d differs in a dibit" % (name, k)
                    assert len(fk) == len(frames) and all(a[:3] == b[:3] and np.array_equal(a[3], b[3]) for a, b in zip(fk, frames)), "%s: run %d differs in a frame" % (name, k)
                    dev[k] = sk.astype(np.float64) - soft.astype(np.float64)
                    runs.append(sk)
                dev_max = np.abs(dev).max(axis=0)
                rms = float(np.sqrt(np.mean(soft.astype(np.float64) ** 2)))
                G = 10.0 * float(np.maximum(1e-5 * rms, 4.0 * dev_max).max())
                s64 = soft.astype(np.float64)
                settled = np.ones(len(soft), bool)
                first = 0
                for b in range(len(cut)):
                    if b == 0 or b in resets:
                        settled[first:first + STARTUP] = False
                    first += int(counts[b])
                margin = float(np.minimum(np.abs(s64), np.abs(np.abs(s64) - float(HIGH_CUT)))[settled].min())
                # the start-up symbols lie at a decision level by construction: what the comparison of their dibits may rely on is asserted on its own — over all
                # nine runs each keeps its sign (none is a zero of either sign in one run and not in another) and its side of the second threshold
                neg = np.stack([r_ < np.float32(0.0) for r_ in runs])
                high = np.stack([np.abs(r_) > HIGH_CUT for r_ in runs])
                zero = np.stack([r_ == np.float32(0.0) for r_ in runs])
                stable = (neg == neg[0]).all(axis=0) & (high == high[0]).all(axis=0) & (zero == zero[0]).all(axis=0)
                assert stable[~settled].all(), "%s: a start-up symbol changes its sign or its side of the threshold under a one-ulp change of the input" % name
                if margin > G and (not all_five or len(frames) == 5):
                    break
                print("%-14s seed %d: margin %.3g against G %.3g, %d frames: another seed" % (name, seed, margin, G, len(frames)))
            else:
                raise SystemExit("%s: no seed gives the margin" % name)
            sl = np.zeros(2 * len(soft), np.uint8)
            sl[0::2] = soft < np.float32(0.0)
            sl[1::2] = np.abs(soft) > HIGH_CUT
            assert np.array_equal(sl, dibits)
            out[name + "_x"] = q
            out[name + "_cut"] = np.asarray(cut, np.int32)
            out[name + "_reset"] = np.asarray(resets, np.int32)
            out[name + "_soft"] = soft
            out[name + "_counts"] = counts
            out[name + "_dibits"] = dibits
            out[name + "_pcl"] = np.fromfile(files[3], np.float32)
            out[name + "_taps"] = np.fromfile(files[4], np.float32)
            out[name + "_ftype"] = np.asarray([f[0] for f in frames], np.int32)
            out[name + "_fstream"] = np.asarray([f[1] for f in frames], np.int32)
            out[name + "_fblock"] = np.asarray([f[2] for f in frames], np.int32)
            out[name + "_frames"] = np.asarray([f[3] for f in frames], np.uint8).reshape(len(frames), 368)
            out[name + "_settled"] = settled.astype(np.uint8)
            out[name + "_startup_sign"] = np.where(settled, 0, np.where(soft < np.float32(0.0), -1, 1)).astype(np.int8)
            out[name + "_dev_max"] = dev_max.astype(np.float32)
            out[name + "_dev_rms"] = np.float64(np.sqrt(np.mean(dev * dev)))
            tab = open(files[7], "rb").read()
            out["scramble"] = np.frombuffer(tab, np.uint8, 368, 0).copy()
            out["interleave"] = np.frombuffer(tab, np.uint16, 368, 368).copy()
            out["sync"] = np.frombuffer(tab, np.uint8, 48, 368 + 736).copy().reshape(3, 16)
            print("%-14s seed %d delay %d: symbols %d, frames %d (types %s, blocks %s), margin %.3g against G %.3g, spread max %.3g rms %.3g, soft rms %.3f" % (
                name, seed, delays[dkey], len(soft), len(frames), list(out[name + "_ftype"]), list(out[name + "_fblock"]), margin, G, dev_max.max(), out[name + "_dev_rms"], rms))
            names.append(name)
        out["names"] = np.asarray(names)
    path = os.path.join(ROOT, "tests", "golden", "m17_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
