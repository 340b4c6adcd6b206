#!/usr/bin/env python3
"""What the WFM demodulator's stereo branch costs on the headline workload (cfg 3: 10 MS/s, 32 WFM VFOs + the 65536-point waterfall branch, pipelined, blocks
resident on the device, zoomed lines delivered and every block's results collected `depth + 1` launches behind its push), with the branch on 0, 1 and all 32
channels (sdrpp_vfo_set_stereo), at two block sizes: 10^6 samples in launch groups of 4 (bench.py's headline shape) and sr / 200 = 50 000 samples (the reference's
own block; 1 250 IF samples per channel and block), one block per launch.

One process, one context per variant, the variants interleaved region by region (box drift shows as scatter, not as a difference); the figure of a variant is
the median over its regions, min .. max beside it — the spread of `0` is the yardstick for the differences.  Per variant: Msamples/s of the input stream, the
tick kernel's own duration per block (HIP events on the launches, regions of their own), the pipeline depth (the result lag in blocks is depth + 1 launches),
the workgroups of the IF chain's role per block (the branch's three job kinds run under it) and the result bytes a block delivers (flag 2: zoomed lines).

    tools/stereo_rate.py [--blocks 120] [--rounds 5] [--out profiles/stereo_rate.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING = 8
SHAPES = [dict(push=1000000, group=4, nvfo=32), dict(push=50000, group=1, nvfo=32)]
VARIANTS = (0, 1, 32)  # channels that carry the branch


class Leg:
    def __init__(self, cfg, variant, push, group, nvfo, x_ring):
        from sdrplusplus_amd import capi, radio, workloads

        self.variant, self.push, self.group = variant, push, group
        self.ctx = ctx = capi.Context(0, max_push=push * group)
        info = workloads.setup(ctx, cfg, dense_fft=True, data_width=1024, nvfo=nvfo)
        self.sr = info["sr"]
        self.vids = info["vids"]
        ctx.set_reference_block(int(self.sr / 200))
        for v, (_m, if_rate, _bw, _c, _x) in list(zip(self.vids, info["plan"]))[:variant]:
            sd, keep = radio.stereo_desc(if_rate)
            ctx.vfo_set_stereo(v, sd, keep)
        ctx.set_pipelined(True, 2)
        if group > 1:
            ctx.set_pipeline_group(group, True)  # (adaptive, as bench.py's headline run)
        self.ptr = [x_ring.data_ptr() + 8 * push * i for i in range(RING)]  # (contiguous blocks: consecutive pushes may share a launch)
        self.res = capi.Result()
        self.pending = []
        self.n = 0
        self.res_bytes = 0
        self.lag = 13 * group
        self.run(4 * group + self.lag)
        self.lag = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1) * group

    def collect(self, tk):
        ctx, L = self.ctx, self.ctx.L
        ctx._chk(L.sdrpp_result_wait(ctx.h, tk, C.byref(self.res)))
        self.res_bytes += int(self.res.n_lines) * int(self.res.data_width) * 4
        ctx._chk(L.sdrpp_result_release(ctx.h, tk))

    def run(self, nblocks):
        ctx = self.ctx
        for _ in range(nblocks):
            ctx.push_device(self.ptr[self.n % RING], self.push)
            self.n += 1
            self.pending.append(ctx.ticket())
            if len(self.pending) > self.lag:
                self.collect(self.pending.pop(0))
        while self.pending:
            self.collect(self.pending.pop(0))
        ctx.sync()

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


def measure(cfg, sh, a, np, torch):
    from sdrplusplus_amd import workloads

    push, group, nvfo = sh["push"], sh["group"], sh["nvfo"]
    x0 = workloads.synth(cfg, push, seed=7, nvfo=nvfo)
    ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
    legs = [Leg(cfg, v, push, group, nvfo, ring) for v in VARIANTS]
    rates = {leg.variant: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            r = leg.timed(a.blocks)
            rates[leg.variant].append(r)
            print("cfg %d round %d  %-8s channels %9.1f MS/s" % (cfg, rnd, leg.variant, r), flush=True)
    ticks = {leg.variant: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            ticks[leg.variant].append(leg.tick_us_per_block(a.blocks))
    rows = []
    for leg in legs:
        rs, ts = sorted(rates[leg.variant]), sorted(ticks[leg.variant])
        st = leg.ctx.pipeline_stats()
        rows.append(dict(cfg=cfg, variant=leg.variant, Msps=round(rs[len(rs) // 2], 1), Msps_min=round(rs[0], 1), Msps_max=round(rs[-1], 1),
                         tick_us=round(ts[len(ts) // 2], 2), tick_us_min=round(ts[0], 2), tick_us_max=round(ts[-1], 2), depth=st["depth"], pass_blocks=st["pass_blocks"],
                         ifc_wgs_per_block=round(st["roles"].get("ifc", 0) / max(1, st["tick_blocks"]), 1), res_bytes_per_block=round(leg.res_bytes / max(1, leg.n), 1)))
        leg.ctx.set_pipelined(False)
        leg.ctx.close()
    print(json.dumps(rows), flush=True)
    na = rows[0]
    table = ["### cfg %d: %d VFOs, push %d, %d blocks per launch, %d regions of %d blocks per variant" % (cfg, nvfo, push, group, a.rounds, a.blocks), "",
             "| stereo channels | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | `ifc` workgroups per block | result bytes per block | blocks as ordinary passes |", "|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        table.append("| %d | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %.1f | %.1f | %d |" % (r["variant"], r["Msps"], r["Msps_min"], r["Msps_max"], r["tick_us"], r["tick_us_min"], r["tick_us_max"], r["depth"],
                                                                                            r["ifc_wgs_per_block"], r["res_bytes_per_block"], r["pass_blocks"]))
    spread = na["tick_us_max"] - na["tick_us_min"]
    for r in rows[1:]:
        diff = r["tick_us"] - na["tick_us"]
        table += ["", "Tick time, %d channels - 0: %+.2f us per block; run-to-run spread of `0` (max - min over its regions): %.2f us — %s." % (r["variant"], diff, spread, "inside the spread" if diff <= spread else "OUTSIDE the spread")]
    table += [""]
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    import numpy as np
    import torch

    table = []
    for sh in SHAPES:
        table += measure(3, sh, a, np, torch)
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
