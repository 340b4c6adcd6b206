#!/usr/bin/env python3
"""What the M17 frame branch (sdrpp_design_m17: the symbol branch with M17's description; sdrpp_vfo_set_framer: slicer, sync search, frame demux) costs.

1. `headline`: the headline workload with no branch and no framer on any channel, this tree against another built checkout (the parent commit), interleaved
   region by region — tools/pager_rate.py's measurement, unchanged:

       tools/m17_rate.py headline --other /path/to/parent/checkout [--rounds 5] [--blocks 120]

2. `m17`: 2.4 MS/s, 64 and 128 RAW VFOs at 14.4 kS/s / 9 kHz, every one with the symbol branch in M17's description, without and with the framer, blocks of
   sr / 200 = 12 000 and of 10^6 samples, one block per launch, pipelined, the results delivered (flag 64 without the framer: soft values and bits; flag 512 with
   it: frame records) and collected `depth + 1` launches behind the push: Msamples/s, the tick's own duration per block, result bytes collected per block.

       tools/m17_rate.py m17 [--rounds 5] [--blocks 60] [--out profiles/m17_rate.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tools"))
RING = 8


def m17_signal(n, sr, seed):
    """a repeating M17 stream frame as 4FSK at 4800 baud around 0 Hz (rectangular symbols: the rate does not depend on the shaping)"""
    import numpy as np

    sys.path.insert(0, os.path.join(HERE, "tests"))
    import m17_ref as R

    r = np.random.default_rng(seed)
    level = {(0, 1): 1.0, (0, 0): 1.0 / 3.0, (1, 0): -1.0 / 3.0, (1, 1): -1.0}
    bits = np.concatenate([[(R.SYNC[1] >> (15 - b)) & 1 for b in range(16)], r.integers(0, 2, 368)])  # (the payload is arbitrary: the framer's work does not depend on it)
    sym = np.array([level[(int(bits[i]), int(bits[i + 1]))] for i in range(0, 384, 2)])
    t = np.arange(n) / sr
    f = 2400.0 * sym[(t * 4800.0).astype(np.int64) % len(sym)]
    return 0.02 * np.exp(1j * 2 * np.pi * np.cumsum(f) / sr)


def m17(a):
    import numpy as np
    import torch
    from sdrplusplus_amd import capi, radio

    sr, if_rate, bw = 2.4e6, 14400.0, 9000.0
    table = []
    for nvfo in (64, 128):
        for push in (12000, 1000000):
            r = np.random.default_rng(5)
            t = np.arange(push) / sr
            base = m17_signal(push, sr, 6)
            x0 = (0.002 * (r.standard_normal(push) + 1j * r.standard_normal(push))).astype(np.complex64)
            offs = [(k - nvfo / 2 + 0.5) * 12500.0 for k in range(nvfo)]
            for o in offs[::8]:
                x0 += (base * np.exp(1j * 2 * np.pi * o * t)).astype(np.complex64)
            ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
            ptr = [ring.data_ptr() + 8 * push * i for i in range(RING)]
            nblocks = a.blocks if push < 100000 else max(8, a.blocks // 6)
            rows = []
            for framer in (False, True):
                ctx = capi.Context(0, max_push=push)
                vids = []
                for o in offs:
                    d, keep = radio.vfo_desc(sr, if_rate, bw, o, "RAW")
                    vids.append(ctx.vfo_add(d, keep))
                    sd, fd, skeep = radio.m17_desc(if_rate)
                    ctx.vfo_set_symbols(vids[-1], sd, True, skeep)
                    if framer:
                        ctx.vfo_set_framer(vids[-1], fd, True, skeep)
                ctx.push_device(ptr[0], push)
                nsym = ctx.vfo_sym_count(vids[0])
                ctx.set_pipelined(True, capi.RESULT_FRAMES if framer else capi.RESULT_SYM)
                res, pending, st = capi.Result(), [], dict(n=0, lag=13, bytes=0, frames=0)

                def collect(tk):
                    ctx._chk(ctx.L.sdrpp_result_wait(ctx.h, tk, C.byref(res)))
                    n = C.c_int()
                    for v in vids:
                        if framer:
                            ctx._chk(ctx.L.sdrpp_result_frames(ctx.h, tk, v, None, C.byref(n)))
                            st["bytes"] += 48 * n.value + 4
                            st["frames"] += n.value
                        else:
                            ctx._chk(ctx.L.sdrpp_result_sym(ctx.h, tk, v, None, None, C.byref(n)))
                            st["bytes"] += 5 * n.value + 4
                    ctx._chk(ctx.L.sdrpp_result_release(ctx.h, tk))

                def run(nb):
                    for _ in range(nb):
                        ctx.push_device(ptr[st["n"] % RING], push)
                        st["n"] += 1
                        pending.append(ctx.ticket())
                        if len(pending) > st["lag"]:
                            collect(pending.pop(0))
                    while pending:
                        collect(pending.pop(0))
                    ctx.sync()

                run(20)
                st["lag"] = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1)
                rates, ticks, used, frames = [], [], 0.0, 0.0
                for rnd in range(a.rounds):
                    st["bytes"], st["frames"], n0 = 0, 0, st["n"]
                    t0 = time.perf_counter()
                    run(nblocks)
                    rates.append(push * nblocks / (time.perf_counter() - t0) / 1e6)
                    used, frames = st["bytes"] / max(1, st["n"] - n0), st["frames"] / max(1, st["n"] - n0)
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
                rows.append(dict(framer=framer, Msps=rates[len(rates) // 2], lo=rates[0], hi=rates[-1], tick=ticks[len(ticks) // 2], tlo=ticks[0], thi=ticks[-1], nsym=nsym, used=used, frames=frames,
                                 pass_blocks=pst["pass_blocks"], depth=pst["depth"]))
                print(json.dumps(rows[-1]), flush=True)
            table += ["### %d RAW VFOs at 14.4 kS/s from 2.4 MS/s, M17 symbol branch on every one, blocks of %d samples (%d symbols per channel), %d regions of %d blocks" % (nvfo, push, rows[0]["nsym"], a.rounds, nblocks), "",
                      "| framer | delivered | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | result bytes collected per block | frames per block | blocks as ordinary passes |",
                      "|---|---|---|---|---|---|---|---|---|---|"]
            for q in rows:
                table.append("| %s | %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %.0f | %.1f | %d |" % ("all %d" % nvfo if q["framer"] else "none", "frame records (512)" if q["framer"] else "soft values and bits (64)",
                                                                                                  q["Msps"], q["lo"], q["hi"], q["tick"], q["tlo"], q["thi"], q["depth"], q["used"], q["frames"], q["pass_blocks"]))
            table.append("")
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["headline", "m17"])
    ap.add_argument("--other", default=None, help="headline: another built checkout of the project (the parent commit)")
    ap.add_argument("--blocks", type=int, default=120)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--leg-timeout", type=int, default=240)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    if a.what == "headline":
        if not a.other:
            sys.exit("headline needs --other")
        import pager_rate

        table = pager_rate.headline(a)
    else:
        sys.path.insert(0, HERE)
        table = m17(a)
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
