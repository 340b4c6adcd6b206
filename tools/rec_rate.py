#!/usr/bin/env python3
"""What delivering the audio costs in the recorder's own format: the headline workload (cfg 3: 32 WFM VFOs + the 65536-point waterfall branch) with
the radio's AF chain to 48 kHz behind every VFO, blocks resident on the device, pipelined with bench.py's block size and launch groups, every block's
results collected `depth + 1` launches behind its push — in three modes:

    f32       result flag 1:  every VFO's AF block as 8-byte float frames
    rec_s16   result flag 16: a recorder sink on every VFO, stereo INT16 (4 bytes per frame)
    rec_m16   result flag 16: the same, mono INT16 (2 bytes per frame)

One process, one context per mode, the modes interleaved region by region (box drift shows as scatter, not as a difference); the figure of a mode is the
median over its regions, as tools/ab_tick.py does.  Per mode: Msamples/s of the input stream, the tick kernel's duration per block (HIP events on the
launches, a region of its own) and the result bytes per block.

    tools/rec_rate.py [--push 1000000] [--group 4] [--blocks 120] [--rounds 5] [--out profiles/recorder_delivery_ab.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = (("f32", 1, None), ("rec_s16", 16, False), ("rec_m16", 16, True))
RING = 8


class Leg:
    def __init__(self, torch, np, label, flags, mono, push, group, x_ring):
        from sdrplusplus_amd import capi, radio, workloads

        self.label, self.flags, self.push, self.group = label, flags, push, group
        self.capi = capi
        self.ctx = ctx = capi.Context(0, max_push=push * group)
        info = workloads.setup(ctx, 3, dense_fft=True, data_width=1024, nvfo=32)
        self.vids = list(info["vids"])
        self.keep = []
        for vid, (m_, r_, _b, _c, _x) in zip(info["vids"], info["plan"]):
            a_, k_ = radio.af_desc(r_, 48000.0, 50e-6 if m_ == "WFM" else None, m_ == "NFM")
            ctx.vfo_set_af(vid, a_, k_)
            self.keep.append(k_)
            if mono is not None:
                ctx.vfo_set_rec(vid, 1.0, mono, capi.REC_INT16, False)
        ctx.set_reference_block(int(workloads.CFG[3]["sr"] / 200))
        ctx.set_pipelined(True, flags)
        if group > 1:
            ctx.set_pipeline_group(group, True)  # (adaptive, as bench.py's headline run)
        self.ptr = [x_ring.data_ptr() + 8 * push * i for i in range(RING)]  # (contiguous blocks: consecutive pushes may share a launch)
        self.res = capi.Result()
        self.info = capi.RecInfo() if flags & 16 else None
        self.pending = []
        self.n = 0
        self.lag = 13 * group
        self.run(4 * group + self.lag)
        self.lag = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1) * group
        self.bytes_per_block = self.measure_bytes()

    def collect(self, tk, count=False):
        ctx, L = self.ctx, self.ctx.L
        ctx._chk(L.sdrpp_result_wait(ctx.h, tk, C.byref(self.res)))
        nbytes = 0
        if self.flags & 1:
            if count:
                nbytes += 8 * sum(self.res.counts[i] for i in range(self.res.n_vfo))
        if self.flags & 16:
            for vid in self.vids:  # (what a host does per recorder: one look-up, the bytes are where they are)
                ctx._chk(L.sdrpp_result_rec(ctx.h, tk, vid, None, C.byref(self.info)))
                if count:
                    nbytes += self.info.frames * self.info.channels * 2
        ctx._chk(L.sdrpp_result_release(ctx.h, tk))
        return nbytes

    def run(self, nblocks, count=False):
        ctx = self.ctx
        total = 0
        for _ in range(nblocks):
            ctx.push_device(self.ptr[self.n % RING], self.push)
            self.n += 1
            self.pending.append(ctx.ticket())
            if len(self.pending) > self.lag:
                total += self.collect(self.pending.pop(0), count)
        while self.pending:
            total += self.collect(self.pending.pop(0), count)
        ctx.sync()
        return total

    def measure_bytes(self):
        n = 4 * self.group
        return self.run(n, count=True) / n

    def timed(self, nblocks):
        t0 = time.perf_counter()
        self.run(nblocks)
        return self.push * nblocks / (time.perf_counter() - t0) / 1e6

    def tick_us_per_block(self, nblocks):
        ctx = self.ctx
        ctx.timing_enable(True, families=[ctx.family_index("tick")])
        self.run(nblocks)
        ms, _n = ctx.timing_read()["tick"]
        ctx.timing_enable(False)
        return ms * 1e3 / nblocks


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--push", type=int, default=1000000)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--blocks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the table (markdown) to this file")
    ap.add_argument("--title", default="this commit")
    ap.add_argument("--modes", default="f32,rec_s16,rec_m16", help="comma-separated subset of the modes (f32 alone also runs on a library without the recorder sink)")
    a = ap.parse_args()
    import numpy as np
    import torch

    from sdrplusplus_amd import workloads

    x0 = workloads.synth(3, a.push, seed=7, nvfo=32)
    ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
    legs = [Leg(torch, np, label, flags, mono, a.push, a.group, ring) for label, flags, mono in MODES if label in a.modes.split(",")]
    rates = {leg.label: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            r = leg.timed(a.blocks)
            rates[leg.label].append(r)
            print("round %d  %-8s %9.1f MS/s" % (rnd, leg.label, r), flush=True)
    rows = []
    for leg in legs:
        rs = sorted(rates[leg.label])
        st = leg.ctx.pipeline_stats()
        rows.append(dict(mode=leg.label, flags=leg.flags, Msps=round(rs[len(rs) // 2], 1), Msps_min=round(rs[0], 1), Msps_max=round(rs[-1], 1),
                         tick_us_per_block=round(leg.tick_us_per_block(a.blocks), 2), result_bytes_per_block=int(leg.bytes_per_block), depth=st["depth"], pass_blocks=st["pass_blocks"]))
        leg.ctx.set_pipelined(False)
        leg.ctx.close()
    print(json.dumps(rows), flush=True)
    table = ["### %s: push %d, %d blocks per launch, %d regions of %d blocks per mode" % (a.title, a.push, a.group, a.rounds, a.blocks), "",
             "| mode | result flags | Msamples/s (median) | min .. max | tick us per block | result bytes per block | depth | blocks as ordinary passes |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        table.append("| %s | %d | %.1f | %.1f .. %.1f | %.2f | %d | %d | %d |" % (r["mode"], r["flags"], r["Msps"], r["Msps_min"], r["Msps_max"], r["tick_us_per_block"], r["result_bytes_per_block"], r["depth"], r["pass_blocks"]))
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n\n")


if __name__ == "__main__":
    main()
