#!/usr/bin/env python3
"""What the Meteor QPSK demodulator (sdrpp_vfo_set_qpsk: root-raised-cosine FIR, AGC, QPSK Costas loop, complex clock recovery, int8 pairs) costs, in the manner
of tools/rds_demod_rate.py.  The headline workload with the demodulator on no channel is measured against the parent commit's tree with tools/ab_tick.py /
`tools/pager_rate.py headline --other <tree>`; this tool measures the demodulator itself:

1, 32 and 128 RAW VFOs at 150 kS/s from 1.2 MS/s, each with the demodulator, in blocks of 240 000 input samples (0.2 s: 30 000 samples and about 14 400 symbols
per channel), ORDINARY passes: wall time per block (the multiple of real time), and the time of the demodulators' two launches per block from the per-family
timers (family `demod`: a RAW bank launches nothing else there) with three descriptions, so that front and loop come apart BY DIFFERENCE:
    module   the module's: 33 taps, omega 2.083
    K1       the same with ONE tap: no filter to speak of — module minus K1 is the front's 32 further taps
    K1w70    that with omega = 70: one symbol per 70 samples instead of per 2.08 — K1 minus K1w70 is MM's walk over the symbols that are gone; what is left is
             the loop's serial pass (AGC, derotation, error, advance) with the chunk loads, the one-tap front and both launches
Clocks are microseconds times the device's reported maximum engine clock (an ASSUMED 2400 MHz where it reports none).

    tools/meteor_rate.py [--blocks 12] [--rounds 3] [--out profiles/meteor_rate.md]"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLOCK_MHZ = 2400.0  # ASSUMED engine clock where the device reports none; every clocks figure scales with it
SR, RATE, PUSH = 1.2e6, 150e3, 240000


def device_clock_mhz():
    try:
        import torch

        khz = int(torch.cuda.get_device_properties(0).clock_rate)
        if khz > 0:
            return khz / 1e3, "the device's reported maximum engine clock"
    except Exception:
        pass
    return CLOCK_MHZ, "ASSUMED, the device reported none"


def describe(kind):
    from sdrplusplus_amd import radio

    d, keep = radio.meteor_desc(rrc_taps=1 if kind != "module" else 33)
    if kind == "K1w70":
        d.omega, d.min_omega, d.max_omega = 70.0, 69.3, 70.7
    return d, keep


def run(nv, kind, blocks, rounds):
    """-> dict(wall us per block (median of rounds), family `demod` us per block, symbols per channel and block)"""
    import numpy as np
    import torch
    from sdrplusplus_amd import capi, radio

    r = np.random.default_rng(3)
    x = (0.05 * (r.standard_normal(PUSH) + 1j * r.standard_normal(PUSH))).astype(np.complex64)
    dev = torch.from_numpy(x.view(np.float32)).to("cuda")
    ctx = capi.Context(0, max_push=PUSH)
    vids = []
    for i in range(nv):
        d, keep = radio.vfo_desc(SR, RATE, RATE, (i - nv / 2 + 0.5) * 7000.0, "RAW")
        vids.append(ctx.vfo_add(d, keep))
        if kind is not None:
            md, mk = describe(kind)
            ctx.vfo_set_qpsk(vids[-1], md, True, mk)
    for _ in range(3):
        ctx.push_device(dev.data_ptr(), PUSH)
    ctx.sync()
    walls = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(blocks):
            ctx.push_device(dev.data_ptr(), PUSH)
        ctx.sync()
        walls.append((time.perf_counter() - t0) * 1e6 / blocks)
    ctx.timing_enable(True, families=[ctx.family_index("demod")])
    for _ in range(blocks):
        ctx.push_device(dev.data_ptr(), PUSH)
    ctx.sync()
    ms, _n = ctx.timing_read()["demod"]
    ctx.timing_enable(False)
    nsym = ctx.vfo_qpsk_count(vids[0]) if kind is not None else 0
    ctx.close()
    walls.sort()
    return dict(nv=nv, kind=kind or "none", wall=walls[len(walls) // 2], wlo=walls[0], whi=walls[-1], demod=ms * 1e3 / blocks, nsym=nsym)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=12)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    mhz, src = device_clock_mhz()
    nin, real_us = int(PUSH * RATE / SR), PUSH / SR * 1e6
    table = ["### RAW VFOs at 150 kS/s from 1.2 MS/s, blocks of %d input samples (%.0f ms; %d samples per channel), ordinary passes, %d rounds of %d blocks" % (PUSH, real_us / 1e3, nin, a.rounds, a.blocks), "",
             "| channels | description | wall us per block (median) | min .. max | x real time | `demod` launches us per block | symbols per channel and block |", "|---|---|---|---|---|---|---|"]
    rows = {}
    for nv in (1, 32, 128):
        for kind in (None, "module", "K1", "K1w70"):
            q = run(nv, kind, a.blocks, a.rounds)
            print(json.dumps(q), flush=True)
            rows[(nv, q["kind"])] = q
            table.append("| %d | %s | %.0f | %.0f .. %.0f | %.1f | %.1f | %d |" % (nv, q["kind"], q["wall"], q["wlo"], q["whi"], real_us / q["wall"], q["demod"], q["nsym"]))
    table += ["", "By difference (family `demod`, us per block; clocks at %.0f MHz: %s):" % (mhz, src), "",
              "| channels | front: module - K1 (32 taps) | per input sample of a channel | MM's walk: K1 - K1w70 | per symbol | rest: K1w70 (serial pass, loads, one-tap front, two launches) | per input sample |", "|---|---|---|---|---|---|---|"]
    for nv in (1, 32, 128):
        m, k1, w = rows[(nv, "module")], rows[(nv, "K1")], rows[(nv, "K1w70")]
        front, walk, rest = m["demod"] - k1["demod"], k1["demod"] - w["demod"], w["demod"]
        dsym = max(1, k1["nsym"] - w["nsym"])
        table.append("| %d | %.1f us | %.0f clocks | %.1f us | %.0f clocks | %.1f us | %.0f clocks |" % (nv, front, front / nin * mhz, walk, walk / dsym * mhz, rest, rest / nin * mhz))
    table.append("")
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
