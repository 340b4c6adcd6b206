#!/usr/bin/env python3
"""What the RDS demodulator (sdrpp_vfo_set_rds_demod: AGC, two Costas loops, band-pass, clock recovery, bits) costs.  The headline workload with the
demodulator on no channel is measured against the parent commit's tree with `tools/pager_rate.py headline --other <tree>` (regions interleaved; tools/ab_tick.py
swaps libraries under one binding, and this binding refuses a library without the new entry points); this tool measures the rest:

`rds`   the headline's 32 WFM VFOs at 10 MS/s (no waterfall branch), every one with its RDS branch, pipelined, one block per launch, results collected `depth + 1`
        launches behind the push: the demodulator on no channel (flag 32: the samples travel), on all 32 with flag 128 alone, and with flags 128 + 32; blocks
        of 10^6 and of sr / 200 samples.  Msamples/s, the tick's own duration, pipeline depth, result bytes collected per block.
`bpsk`  128 RAW VFOs at 5 kS/s from 500 kS/s with a source-1 demodulator each (and the same bank without), blocks of sr / 200 and of 10^6 samples; and, from
        ordinary passes timed per kernel family, the time of the demodulators' launch per block (family `demod`: a RAW bank launches nothing else there),
        divided by the samples a wavefront walks per block: clocks per input sample of the job, all three passes together.

`passes` the same 128 channels in 10^6-sample blocks (10 000 samples per channel), ordinary passes, family `demod`, with three descriptions, and the job's passes BY
        DIFFERENCE: the radio's; the same with ONE tap (no parallel pass to speak of, no window to move); and that with omega = 64 (one symbol per chunk instead of
        fifteen: a fifteenth of MM's walk and of its bank reads).  What is left is the two serial passes (with the load and the launch), which no description separates.

    tools/rds_demod_rate.py rds|bpsk|passes [--rounds 3] [--blocks 60] [--out profiles/rds_demod_rate.md]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RING = 8
CLOCK_MHZ = 2400.0  # ASSUMED engine clock where the device reports none (device_clock_mhz); every clocks-per-sample figure scales with it


def device_clock_mhz():
    """the device's reported maximum engine clock -> (MHz, where the figure comes from)"""
    try:
        import torch

        khz = int(torch.cuda.get_device_properties(0).clock_rate)
        if khz > 0:
            return khz / 1e3, "the device's reported maximum engine clock"
    except Exception:
        pass
    return CLOCK_MHZ, "ASSUMED, the device reported none"


def measure(ctx, vids, ptr, push, nblocks, rounds, collect_one, collecting):
    """pipelined, one block per launch -> dict(Msps median / lo / hi, tick us, depth, bytes per block, blocks as ordinary passes)"""
    from sdrplusplus_amd import capi

    res, pending, st = capi.Result(), [], dict(n=0, lag=13, bytes=0)

    def collect(tk):
        ctx._chk(ctx.L.sdrpp_result_wait(ctx.h, tk, C.byref(res)))
        for v in vids:
            st["bytes"] += collect_one(tk, v)
        ctx._chk(ctx.L.sdrpp_result_release(ctx.h, tk))

    def run(nb):
        for _ in range(nb):
            ctx.push_device(ptr[st["n"] % RING], push)
            st["n"] += 1
            pending.append(ctx.ticket())
            if collecting and len(pending) > st["lag"]:
                collect(pending.pop(0))
        while collecting and pending:
            collect(pending.pop(0))
        del pending[:]
        ctx.sync()

    run(20)
    st["lag"] = min(capi.RESULT_SLOTS - 2, int(ctx.pipeline_stats()["depth"]) + 1)
    rates, ticks, used = [], [], 0.0
    for _ in range(rounds):
        st["bytes"], n0 = 0, st["n"]
        t0 = time.perf_counter()
        run(nblocks)
        rates.append(push * nblocks / (time.perf_counter() - t0) / 1e6)
        used = st["bytes"] / max(1, st["n"] - n0)
    for _ in range(rounds):
        ctx.timing_enable(True, families=[ctx.family_index("tick")])
        run(nblocks)
        ms, _n = ctx.timing_read()["tick"]
        ctx.timing_enable(False)
        ticks.append(ms * 1e3 / nblocks)
    pst = ctx.pipeline_stats()
    rates.sort()
    ticks.sort()
    return dict(Msps=rates[len(rates) // 2], lo=rates[0], hi=rates[-1], tick=ticks[len(ticks) // 2], tlo=ticks[0], thi=ticks[-1], depth=pst["depth"], used=used, pass_blocks=pst["pass_blocks"])


def ring_of(x0, push):
    import numpy as np
    import torch

    ring = torch.from_numpy(np.concatenate([np.roll(x0, 1009 * i) for i in range(RING)]).view(np.float32)).to("cuda")
    return ring, [ring.data_ptr() + 8 * push * i for i in range(RING)]


HEAD = ["| demodulator | result flags | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | result bytes collected per block | blocks as ordinary passes |", "|---|---|---|---|---|---|---|---|---|"]


def line(label, flags, q):
    return "| %s | %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %.0f | %d |" % (label, flags, q["Msps"], q["lo"], q["hi"], q["tick"], q["tlo"], q["thi"], q["depth"], q["used"], q["pass_blocks"])


def rds(a):
    from sdrplusplus_amd import capi, radio, workloads

    table = []
    sr = workloads.CFG[3]["sr"]
    for push in (1000000, int(sr / 200)):
        x0 = workloads.synth(3, push, seed=7, nvfo=32)
        ring, ptr = ring_of(x0, push)
        nblocks = a.blocks if push < 100000 else max(8, a.blocks // 4)
        table += ["### 32 WFM VFOs at 10 MS/s, each with its RDS branch, blocks of %d samples, %d regions of %d blocks" % (push, a.rounds, nblocks), ""] + HEAD
        for label, demod, flags in (("none", False, capi.RESULT_RDS), ("all 32", True, capi.RESULT_RDS_BITS), ("all 32", True, capi.RESULT_RDS_BITS | capi.RESULT_RDS)):
            ctx = capi.Context(0, max_push=push)
            info = workloads.setup(ctx, 3, dense_fft=True, data_width=1024, nvfo=32, fft=False)
            for vid, (_m, if_rate, _b, _c, _x) in zip(info["vids"], info["plan"]):
                d, k = radio.rds_desc(if_rate)
                ctx.vfo_set_rds(vid, d, True, k)
                if demod:
                    rd, rk = radio.rds_demod_desc(5000.0, 0)
                    ctx.vfo_set_rds_demod(vid, rd, True, rk)
            ctx.set_pipelined(True, flags)
            n = C.c_int()

            def collect_one(tk, v, flags=flags):
                got = 0
                if flags & capi.RESULT_RDS:
                    ctx._chk(ctx.L.sdrpp_result_rds(ctx.h, tk, v, None, C.byref(n)))
                    got += 8 * n.value
                if flags & capi.RESULT_RDS_BITS:
                    ctx._chk(ctx.L.sdrpp_result_rds_bits(ctx.h, tk, v, None, None, C.byref(n)))
                    got += 5 * n.value + 4
                return got

            q = measure(ctx, info["vids"], ptr, push, nblocks, a.rounds, collect_one, True)
            ctx.set_pipelined(False)
            ctx.close()
            print(json.dumps(q), flush=True)
            table.append(line(label, " + ".join(s for s, f in (("128", capi.RESULT_RDS_BITS), ("32", capi.RESULT_RDS)) if flags & f), q))
        table.append("")
        del ring
    return table


def bpsk(a):
    import numpy as np
    from sdrplusplus_amd import capi, radio

    sr, rate, bw, nvfo = 500e3, 5e3, 3e3, 128
    table = []
    for push in (int(sr / 200), 1000000):
        r = np.random.default_rng(5)
        t = np.arange(push) / sr
        bits = np.bitwise_xor.accumulate(r.integers(0, 2, int(push / sr * 1187.5) + 2))
        sym = t * 1187.5
        k = np.floor(sym).astype(np.int64)
        base = 0.02 * np.where(bits[k] == 1, 1.0, -1.0) * np.sin(2 * np.pi * (sym - k))
        x0 = (0.002 * (r.standard_normal(push) + 1j * r.standard_normal(push))).astype(np.complex64)
        offs = [(i - nvfo / 2 + 0.5) * 3900.0 for i in range(nvfo)]
        for o in offs[::8]:
            x0 += (base * np.exp(1j * 2 * np.pi * o * t)).astype(np.complex64)
        ring, ptr = ring_of(x0, push)
        nblocks = a.blocks if push < 100000 else max(8, a.blocks // 4)
        rows = []
        for demod in (False, True):
            ctx = capi.Context(0, max_push=push)
            vids = []
            for o in offs:
                d, keep = radio.vfo_desc(sr, rate, bw, o, "RAW")
                vids.append(ctx.vfo_add(d, keep))
                if demod:
                    rd, rk = radio.rds_demod_desc(rate, 1)
                    ctx.vfo_set_rds_demod(vids[-1], rd, True, rk)
            demod_us, nsym = 0.0, 0
            if demod:  # ordinary passes, per-family timers: `demod` is the demodulators' launch
                for i in range(3):
                    ctx.push_device(ptr[i % RING], push)
                ctx.timing_enable(True, families=[ctx.family_index("demod")])
                for i in range(nblocks):
                    ctx.push_device(ptr[i % RING], push)
                ctx.sync()
                ms, _n = ctx.timing_read()["demod"]
                ctx.timing_enable(False)
                demod_us = ms * 1e3 / nblocks
                nsym = ctx.vfo_rds_demod_count(vids[0])
            ctx.set_pipelined(True, capi.RESULT_RDS_BITS if demod else 0)
            n = C.c_int()

            def collect_one(tk, v):
                ctx._chk(ctx.L.sdrpp_result_rds_bits(ctx.h, tk, v, None, None, C.byref(n)))
                return 5 * n.value + 4

            q = measure(ctx, vids, ptr, push, nblocks, a.rounds, collect_one, demod)
            q.update(demod_us=demod_us, nsym=nsym)
            ctx.set_pipelined(False)
            ctx.close()
            print(json.dumps(q), flush=True)
            rows.append(q)
        nin = push // 100
        table += ["### %d RAW VFOs at 5 kS/s from 500 kS/s, blocks of %d samples (%d samples, %d symbols per channel), %d regions of %d blocks" % (nvfo, push, nin, rows[1]["nsym"], a.rounds, nblocks), ""] + HEAD
        table += [line("none", "-", rows[0]), line("all %d" % nvfo, "128", rows[1]), ""]
        q = rows[1]
        mhz, src = device_clock_mhz()
        per = q["demod_us"] / max(1, nin)
        table += ["Ordinary passes, family `demod` (one launch of %d wavefront jobs, four to a workgroup): %.1f us per block; %d samples per wavefront and block: %.3f us = about %.0f clocks per input sample "
                  "and wavefront, all three passes together, launch included (at %.0f MHz: %s)." % (nvfo, q["demod_us"], nin, per, per * mhz, mhz, src), ""]
        del ring
    return table


def passes(a):
    import numpy as np
    from sdrplusplus_amd import capi, radio

    sr, rate, bw, nvfo, push = 500e3, 5e3, 3e3, 128, 1000000
    mhz, src = device_clock_mhz()
    r = np.random.default_rng(5)
    x0 = (0.02 * (r.standard_normal(push) + 1j * r.standard_normal(push))).astype(np.complex64)
    ring, ptr = ring_of(x0, push)
    offs = [(i - nvfo / 2 + 0.5) * 3900.0 for i in range(nvfo)]
    nin, nblocks = push // 100, 6
    one = np.array([1.0 + 0.0j], np.complex64)

    def describe(kind):
        rd, rk = radio.rds_demod_desc(rate, 1)
        if kind != "radio":
            rd.n_taps = 1
            rd.taps = one.view(np.float32).ctypes.data_as(capi.c_float_p)
        if kind == "one tap, omega 64":
            rd.omega, rd.min_omega, rd.max_omega = 64.0, 63.4, 64.6
        return rd, rk

    got = {}
    for kind in ("radio", "one tap", "one tap, omega 64"):
        ctx = capi.Context(0, max_push=push)
        vids = []
        for o in offs:
            d, keep = radio.vfo_desc(sr, rate, bw, o, "RAW")
            vids.append(ctx.vfo_add(d, keep))
            rd, rk = describe(kind)
            ctx.vfo_set_rds_demod(vids[-1], rd, True, rk)
        for i in range(3):
            ctx.push_device(ptr[i % RING], push)
        us = []
        for _ in range(a.rounds):
            ctx.timing_enable(True, families=[ctx.family_index("demod")])
            for i in range(nblocks):
                ctx.push_device(ptr[i % RING], push)
            ctx.sync()
            ms, _n = ctx.timing_read()["demod"]
            ctx.timing_enable(False)
            us.append(ms * 1e3 / nblocks)
        nsym = ctx.vfo_rds_demod_count(vids[0])
        ctx.close()
        us.sort()
        got[kind] = dict(us=us[len(us) // 2], lo=us[0], hi=us[-1], nsym=nsym)
        print(kind, json.dumps(got[kind]), flush=True)
    clk = lambda u: u / nin * mhz
    A, B, Cc = got["radio"], got["one tap"], got["one tap, omega 64"]
    table = ["### The job's passes by difference: %d RAW VFOs at 5 kS/s, blocks of %d samples (%d per channel), ordinary passes, family `demod`, %d regions of %d blocks; %.0f MHz (%s)" % (nvfo, push, nin, a.rounds, nblocks, mhz, src), "",
             "| description | us per block (median) | min .. max | symbols per channel and block | clocks per input sample and wavefront |", "|---|---|---|---|---|"]
    for kind in ("radio", "one tap", "one tap, omega 64"):
        q = got[kind]
        table.append("| %s | %.1f | %.1f .. %.1f | %d | %.0f |" % (kind, q["us"], q["lo"], q["hi"], q["nsym"], clk(q["us"])))
    walk_sym = (B["us"] - Cc["us"]) / max(1, B["nsym"] - Cc["nsym"])  # us per symbol walked
    table += ["", "By difference, clocks per input sample and wavefront: parallel pass (190 taps against 1, window move included) %.0f; MM's walk, slicer and decoder with the scalar bank-row read on the symbol's chain %.0f "
              "(%.0f clocks per SYMBOL: the cost of the through-the-cache bank variant lies inside this figure); the two serial passes together with the chunk loads and the launch, not separated by any description: %.0f "
              "(the one-tap, omega-64 run less the %.0f its own %d symbols cost)." % (
                  clk(A["us"] - B["us"]), clk(walk_sym * B["nsym"]), walk_sym * mhz, clk(Cc["us"] - walk_sym * Cc["nsym"]), clk(walk_sym * Cc["nsym"]), Cc["nsym"]), ""]
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["rds", "bpsk", "passes"])
    ap.add_argument("--blocks", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    a = ap.parse_args()
    sys.path.insert(0, HERE)
    table = rds(a) if a.what == "rds" else (bpsk(a) if a.what == "bpsk" else passes(a))
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")


if __name__ == "__main__":
    main()
