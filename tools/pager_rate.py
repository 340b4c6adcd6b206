#!/usr/bin/env python3
"""What the symbol branch (sdrpp_vfo_set_symbols: discriminator, shaping FIR, Mueller-Mueller clock recovery) costs.

1. `headline`: the headline workload (cfg 3: 10 MS/s, 32 WFM VFOs + the 65536-point waterfall branch, pipelined, 10^6-sample blocks in launch groups of 4,
   blocks resident on the device) with the branch on NO channel, this tree against another checkout of the project (the parent commit, built), each region
   a process of its own, the two trees interleaved region by region: median, min .. max per tree — the spread of either is the yardstick for the difference.

       tools/pager_rate.py headline --other /path/to/parent/checkout [--rounds 5] [--blocks 120]

2. `pager`: 2.4 MS/s, 64 and 128 RAW VFOs at 24 kS/s / 12.5 kHz, every one with the branch at 2400 baud (and the same bank without it), blocks of sr / 200 =
   12 000 and of 10^6 samples, one block per launch, pipelined with the symbols delivered (result flag 64) and collected `depth + 1` launches behind the push:
   Msamples/s, the tick's own duration per block, result bytes per block — and, from ordinary passes of the same bank timed per kernel family, the time of the
   branch's two launches per block (family `demod`: front, then loop; a RAW bank launches nothing else there), divided by the symbols a lane of the loop walks
   per block: an upper bound of the loop's cost per symbol and wavefront (the front's share is in it).

       tools/pager_rate.py pager [--rounds 5] [--blocks 60] [--out profiles/pager_rate.md]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 8


def leg_headline(a):
    """one region of the headline workload in this process -> JSON"""
    import numpy as np
    import torch
    from sdrplusplus_amd import capi, workloads

    push, group = 1000000, 4
    ctx = capi.Context(0, max_push=push * group)
    info = workloads.setup(ctx, 3, dense_fft=True, data_width=1024, nvfo=32)
    ctx.set_reference_block(int(info["sr"] / 200))
    ctx.set_pipelined(True, 2)
    ctx.set_pipeline_group(group, True)
    x0 = workloads.synth(3, push, seed=7, nvfo=32)
    ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
    ptr = [ring.data_ptr() + 8 * push * i for i in range(RING)]
    res, pending, state = capi.Result(), [], dict(n=0, lag=13 * group)

    def run(nblocks):
        for _ in range(nblocks):
            ctx.push_device(ptr[state["n"] % RING], push)
            state["n"] += 1
            pending.append(ctx.ticket())
            if len(pending) > state["lag"]:
                tk = pending.pop(0)
                ctx._chk(ctx.L.sdrpp_result_wait(ctx.h, tk, C.byref(res)))
                ctx._chk(ctx.L.sdrpp_result_release(ctx.h, tk))
        while pending:
            tk = pending.pop(0)
            ctx._chk(ctx.L.sdrpp_result_wait(ctx.h, tk, C.byref(res)))
            ctx._chk(ctx.L.sdrpp_result_release(ctx.h, tk))
        ctx.sync()

    run(4 * group + state["lag"])
    state["lag"] = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1) * group
    t0 = time.perf_counter()
    run(a.blocks)
    msps = push * a.blocks / (time.perf_counter() - t0) / 1e6
    ctx.timing_enable(True, families=[ctx.family_index("tick")])
    run(a.blocks)
    ms, _n = ctx.timing_read()["tick"]
    ctx.timing_enable(False)
    ctx.set_pipelined(False)
    ctx.close()
    print(json.dumps(dict(Msps=msps, tick_us=ms * 1e3 / a.blocks)), flush=True)


def headline(a):
    trees = [("this", HERE), ("other", os.path.abspath(a.other))]
    got = {k: [] for k, _ in trees}
    for rnd in range(a.rounds):
        for name, tree in trees:
            env = dict(os.environ, PYTHONPATH=tree)
            r = subprocess.run([sys.executable, os.path.join(HERE, "tools", "pager_rate.py"), "_leg_headline", "--blocks", str(a.blocks)], env=env, cwd=tree, capture_output=True, text=True, timeout=a.leg_timeout)
            if r.returncode != 0:
                sys.exit("region failed (%s, exit %d): stopping\n%s" % (name, r.returncode, r.stderr[-2000:]))
            row = json.loads(r.stdout.strip().splitlines()[-1])
            got[name].append(row)
            print("round %d %-5s %8.1f MS/s  tick %7.2f us per block" % (rnd, name, row["Msps"], row["tick_us"]), flush=True)
    table = ["### headline workload (cfg 3, 32 WFM VFOs + waterfall, 10^6-sample blocks, groups of 4), no symbol branch attached: %d regions of %d blocks per tree, interleaved" % (a.rounds, a.blocks), "",
             "| tree | Msamples/s (median) | min .. max | tick us per block (median) | min .. max |", "|---|---|---|---|---|"]
    med = {}
    for name, _ in trees:
        rs, ts = sorted(q["Msps"] for q in got[name]), sorted(q["tick_us"] for q in got[name])
        med[name] = (rs[len(rs) // 2], rs[0], rs[-1], ts[len(ts) // 2], ts[0], ts[-1])
        table.append("| %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f |" % ((name,) + med[name]))
    spread = max(med["other"][5] - med["other"][4], med["this"][5] - med["this"][4])
    diff = med["this"][3] - med["other"][3]
    table += ["", "Tick time, this - other: %+.2f us per block; run-to-run spread (max - min over a tree's regions, the larger of the two): %.2f us — %s." % (diff, spread, "inside the spread" if abs(diff) <= spread else "OUTSIDE the spread"), ""]
    return table


def pager(a):
    import numpy as np
    import torch
    from sdrplusplus_amd import capi, radio

    sr, if_rate, bw, baud = 2.4e6, 24e3, 12.5e3, 2400.0
    table = []
    for nvfo in (64, 128):
        for push in (12000, 1000000):
            r = np.random.default_rng(5)
            t = np.arange(push) / sr
            bits = r.integers(0, 2, int(push / sr * baud) + 2)
            f = np.where(bits[(t * baud).astype(np.int64)] == 1, 4500.0, -4500.0)
            base = 0.02 * np.exp(1j * 2 * np.pi * np.cumsum(f) / sr)
            x0 = (0.002 * (r.standard_normal(push) + 1j * r.standard_normal(push))).astype(np.complex64)
            offs = [(k - nvfo / 2 + 0.5) * 12500.0 for k in range(nvfo)]
            for o in offs[::8]:
                x0 += (base * np.exp(1j * 2 * np.pi * o * t)).astype(np.complex64)
            ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
            ptr = [ring.data_ptr() + 8 * push * i for i in range(RING)]
            nblocks = a.blocks if push < 100000 else max(8, a.blocks // 6)
            rows = []
            for sym in (False, True):
                ctx = capi.Context(0, max_push=push)
                vids = []
                for o in offs:
                    d, keep = radio.vfo_desc(sr, if_rate, bw, o, "RAW")
                    vids.append(ctx.vfo_add(d, keep))
                    if sym:
                        sd, skeep = radio.pager_desc(if_rate, baud)
                        ctx.vfo_set_symbols(vids[-1], sd, True, skeep)
                # ordinary passes, per-family timers: `demod` is the branch's two launches
                demod_us, nsym = 0.0, 0
                if sym:
                    for i in range(3):
                        ctx.push_device(ptr[i % RING], push)
                    ctx.timing_enable(True, families=[ctx.family_index("demod")])
                    for i in range(nblocks):
                        ctx.push_device(ptr[i % RING], push)
                    ctx.sync()
                    ms, _n = ctx.timing_read()["demod"]
                    ctx.timing_enable(False)
                    demod_us = ms * 1e3 / nblocks
                    nsym = ctx.vfo_sym_count(vids[0])
                ctx.set_pipelined(True, capi.RESULT_SYM if sym else 0)
                res, pending, st = capi.Result(), [], dict(n=0, lag=13, bytes=0)

                def run(nb):
                    for _ in range(nb):
                        ctx.push_device(ptr[st["n"] % RING], push)
                        st["n"] += 1
                        pending.append(ctx.ticket())
                        if sym and len(pending) > st["lag"]:
                            collect(pending.pop(0))
                    while sym and pending:
                        collect(pending.pop(0))
                    del pending[:]
                    ctx.sync()

                def collect(tk):
                    ctx._chk(ctx.L.sdrpp_result_wait(ctx.h, tk, C.byref(res)))
                    n = C.c_int()
                    for v in vids:
                        ctx._chk(ctx.L.sdrpp_result_sym(ctx.h, tk, v, None, None, C.byref(n)))
                        st["bytes"] += 5 * n.value + 4
                    ctx._chk(ctx.L.sdrpp_result_release(ctx.h, tk))

                run(20)
                st["lag"] = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1)
                rates, ticks = [], []
                for rnd in range(a.rounds):
                    st["bytes"], n0 = 0, st["n"]
                    t0 = time.perf_counter()
                    run(nblocks)
                    rates.append(push * nblocks / (time.perf_counter() - t0) / 1e6)
                    used = st["bytes"] / max(1, st["n"] - n0)
                for rnd in range(a.rounds):
                    ctx.timing_enable(True, families=[ctx.family_index("tick")])
                    run(nblocks)
                    ms, _n = ctx.timing_read()["tick"]
                    ctx.timing_enable(False)
                    ticks.append(ms * 1e3 / nblocks)
                pst = ctx.pipeline_stats()
                ctx.set_pipelined(False)
                ctx.close()
                rates.sort()
                ticks.sort()
                rows.append(dict(sym=sym, Msps=rates[len(rates) // 2], lo=rates[0], hi=rates[-1], tick=ticks[len(ticks) // 2], tlo=ticks[0], thi=ticks[-1], demod_us=demod_us, nsym=nsym,
                                 used=used, pass_blocks=pst["pass_blocks"], depth=pst["depth"]))
                print(json.dumps(rows[-1]), flush=True)
            table += ["### %d RAW VFOs at 24 kS/s from 2.4 MS/s, blocks of %d samples (%d IF samples, %d symbols per channel), %d regions of %d blocks" % (nvfo, push, push // 100, rows[1]["nsym"], a.rounds, nblocks), "",
                      "| symbol branch | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | symbol bytes collected per block | blocks as ordinary passes |", "|---|---|---|---|---|---|---|---|"]
            for q in rows:
                table.append("| %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %.0f | %d |" % ("all %d" % nvfo if q["sym"] else "none", q["Msps"], q["lo"], q["hi"], q["tick"], q["tlo"], q["thi"], q["depth"], q["used"], q["pass_blocks"]))
            q = rows[1]
            table += ["", "Ordinary passes, family `demod` (front launch + loop launch, %d loop wavefronts of up to 64 lanes): %.1f us per block; %d symbols per lane and block: at most %.3f us per symbol and wavefront." % (
                (nvfo + 63) // 64, q["demod_us"], q["nsym"], q["demod_us"] / max(1, q["nsym"])), ""]
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["headline", "pager", "_leg_headline"])
    ap.add_argument("--other", default=None, help="headline: another built checkout of the project (the parent commit)")
    ap.add_argument("--blocks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    if a.what == "_leg_headline":
        return leg_headline(a)
    if a.what == "headline":
        if not a.other:
            sys.exit("headline needs --other")
        table = headline(a)
    else:
        sys.path.insert(0, HERE)
        table = pager(a)
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
