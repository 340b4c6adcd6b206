#!/usr/bin/env python3
"""What metering every VFO on every line costs: a pipelined run, blocks resident on the device, zoomed lines delivered (result flag 2) and every block's
results collected `depth + 1` launches behind its push — for the headline workload (cfg 3: 32 WFM VFOs + the 65536-point waterfall branch, bench.py's block
size and launch groups) and cfg 4 (128 VFOs, 2^20-point FFT, one block per launch) — in three variants:

    A  none     no table of meters
    B  table    sdrpp_wf_set_meters with one band per VFO: the meters arrive with every block's results (sdrpp_result_meters)
    C  queries  what there was before: a history ring, and sdrpp_wf_signal_info once per VFO after each block (every call drains the pipeline)

One process, one context per variant, the variants interleaved region by region (box drift shows as scatter, not as a difference); the figure of a variant is
the median over its regions, min .. max beside it — the spread of A is the yardstick for the difference B - A.  Per variant: Msamples/s of the input stream,
the tick kernel's own duration per block (HIP events on the launches, a region of its own) and the workgroups of `wf_ring` per block (for B: its meter form, which runs one level behind the lines).

    tools/meter_rate.py [--cfgs 3,4] [--blocks 120] [--rounds 7] [--out profiles/meters_rate.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING = 8
SHAPES = {3: dict(push=1000000, group=4, nvfo=32), 4: dict(push=1000000, group=1, nvfo=128)}
VARIANTS = ("none", "table", "queries")


class Leg:
    def __init__(self, cfg, variant, push, group, nvfo, x_ring):
        from sdrplusplus_amd import capi, radio, workloads

        self.variant, self.push, self.group = variant, push, group
        self.ctx = ctx = capi.Context(0, max_push=push * group)
        info = workloads.setup(ctx, cfg, dense_fft=True, data_width=1024, nvfo=nvfo)
        self.sr = info["sr"]
        self.bands = radio.meter_table([(centre, bw) for _m, _r, bw, centre, _c in info["plan"]])
        ctx.set_reference_block(int(self.sr / 200))
        if variant == "table":
            ctx.wf_set_meters(self.bands, self.sr)
        if variant == "queries":
            ctx.wf_configure(4)
        ctx.set_pipelined(True, 2)
        if group > 1:
            ctx.set_pipeline_group(group, True)  # (adaptive, as bench.py's headline run)
        self.ptr = [x_ring.data_ptr() + 8 * push * i for i in range(RING)]  # (contiguous blocks: consecutive pushes may share a launch)
        self.res = capi.Result()
        self.pending = []
        self.n = 0
        self.lag = 13 * group
        self.run(4 * group + self.lag)
        self.lag = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1) * group

    def collect(self, tk):
        ctx, L = self.ctx, self.ctx.L
        ctx._chk(L.sdrpp_result_wait(ctx.h, tk, C.byref(self.res)))
        if self.variant == "table":
            data, nl, nm = C.POINTER(C.c_float)(), C.c_int(), C.c_int()
            ctx._chk(L.sdrpp_result_meters(ctx.h, tk, C.byref(data), C.byref(nl), C.byref(nm)))
        ctx._chk(L.sdrpp_result_release(ctx.h, tk))

    def run(self, nblocks):
        ctx = self.ctx
        a, b = C.c_float(), C.c_float()
        for _ in range(nblocks):
            ctx.push_device(self.ptr[self.n % RING], self.push)
            self.n += 1
            self.pending.append(ctx.ticket())
            if self.variant == "queries":
                for centre, bw in self.bands:
                    ctx._chk(ctx.L.sdrpp_wf_signal_info(ctx.h, centre, bw, self.sr, C.byref(a), C.byref(b)))
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


def measure(cfg, a, np, torch):
    from sdrplusplus_amd import workloads

    sh = SHAPES[cfg]
    push, group, nvfo = sh["push"], sh["group"], sh["nvfo"]
    x0 = workloads.synth(cfg, push, seed=7, nvfo=nvfo)
    ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
    legs = [Leg(cfg, v, push, group, nvfo, ring) for v in VARIANTS]
    rates = {leg.variant: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            nb = a.blocks if leg.variant != "queries" else max(group * 4, a.blocks // 4)  # (every query is a drain: a quarter of the blocks says as much)
            r = leg.timed(nb)
            rates[leg.variant].append(r)
            print("cfg %d round %d  %-8s %9.1f MS/s" % (cfg, rnd, leg.variant, r), flush=True)
    ticks = {leg.variant: [] for leg in legs}
    for rnd in range(a.rounds):
        for leg in legs:
            ticks[leg.variant].append(leg.tick_us_per_block(a.blocks if leg.variant != "queries" else max(group * 4, a.blocks // 4)))
    rows = []
    for leg in legs:
        rs, ts = sorted(rates[leg.variant]), sorted(ticks[leg.variant])
        st = leg.ctx.pipeline_stats()
        rows.append(dict(cfg=cfg, variant=leg.variant, Msps=round(rs[len(rs) // 2], 1), Msps_min=round(rs[0], 1), Msps_max=round(rs[-1], 1),
                         tick_us=round(ts[len(ts) // 2], 2), tick_us_min=round(ts[0], 2), tick_us_max=round(ts[-1], 2), depth=st["depth"], pass_blocks=st["pass_blocks"],
                         meter_wgs_per_block=round(st["roles"].get("wf_ring", 0) / max(1, st["tick_blocks"]), 1)))
        leg.ctx.set_pipelined(False)
        leg.ctx.close()
    print(json.dumps(rows), flush=True)
    na, nb = rows[0], rows[1]
    table = ["### cfg %d: %d VFOs, push %d, %d blocks per launch, %d regions of %d blocks per variant" % (cfg, nvfo, push, group, a.rounds, a.blocks), "",
             "| variant | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | `wf_ring` workgroups per block (table: its meter form; queries: the ring store) | blocks as ordinary passes |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        table.append("| %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %.1f | %d |" % (r["variant"], r["Msps"], r["Msps_min"], r["Msps_max"], r["tick_us"], r["tick_us_min"], r["tick_us_max"], r["depth"],
                                                                                     r["meter_wgs_per_block"], r["pass_blocks"]))
    spread = na["tick_us_max"] - na["tick_us_min"]
    diff = nb["tick_us"] - na["tick_us"]
    table += ["", "Tick time, table - none: %+.2f us per block; run-to-run spread of `none` (max - min over its regions): %.2f us — %s." % (diff, spread, "inside the spread" if diff <= spread else "OUTSIDE the spread"), ""]
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfgs", default="3,4")
    ap.add_argument("--blocks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    import numpy as np
    import torch

    table = []
    for cfg in [int(c) for c in a.cfgs.split(",")]:
        table += measure(cfg, a, np, torch)
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
