#!/usr/bin/env python3
"""What a bank of CW channels costs in a wide capture, and whether plan 8192's first stage (/128, 726 taps) belongs on the matrix cores: an A / B of library
builds on ONE box.  Workload: N CW VFOs (3 kS/s, bandwidth 200 Hz, tone 800 Hz) spread over the capture, pipelined, blocks resident on the device, outputs
left there; per variant the ingest rate and the tick kernel's own duration (HIP events on the launches).

    tools/cw_rate.py --out profiles/cw_rate.md  parent=libsdrpp_gpu_parent.so,demod=USB  new=libsdrpp_gpu.so

A variant is  label=<library under sdrplusplus_amd/csrc, or an absolute path>[,demod=USB].  demod=USB feeds a library that does not know SDRPP_DEMOD_CW the
same descriptors with the demodulator code of USB and the tone in ssb_phase_delta: the same arithmetic (CW is SSB(USB, 2 * tone)), so a build of the commit
before CW can stand on the other side — there the /128 stage runs in the direct VALU form (s1d_1).  The library switch is a switch of THIS TOOL
(capi.DEFAULT_LIB, as tools/ab_tick.py); every measurement is a process of its own, the variants interleaved round by round so that box drift shows as
scatter, not as a difference.  The figure of a variant is the median over its rounds, min .. max beside it; the matrix form is worth keeping only where its
median tick duration lies below the parent's by more than the parent's own run-to-run spread (max - min), and the tool prints both.

Rows: 128 VFOs at 61.44 MS/s (plan 8192, then 2 / 5) with blocks of 307 200 and 10^6 samples; 32 VFOs at 10 MS/s (plan 2048, then 3000 / 4883) with 10^6."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = [(61.44e6, 128, 307200), (61.44e6, 128, 1000000), (10e6, 32, 1000000)]


def child(sr, nvfo, push, lib, nblocks, demod):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from sdrplusplus_amd import capi, radio

    capi.DEFAULT_LIB = lib if os.path.isabs(lib) else os.path.join(ROOT, "sdrplusplus_amd", "csrc", lib)
    ctx = capi.Context(0, max_push=push)
    if int(sr / 200) < push:
        ctx.set_reference_block(int(sr / 200))
    offs = [((k + 0.5) / nvfo - 0.5) * 0.8 * sr + 13.0 * k for k in range(nvfo)]
    for f in offs:
        d, keep = radio.vfo_desc(sr, 3000.0, 200.0, f, "CW")
        if demod == "USB":
            d.demod = capi.DEMOD_USB
        ctx.vfo_add(d, keep)
    r = np.random.default_rng(7)
    t = np.arange(push, dtype=np.float64) / sr
    x0 = (r.standard_normal(push) + 1j * r.standard_normal(push)) * 1e-3
    for f in offs[::max(1, nvfo // 8)]:
        x0 += 0.05 * np.exp(2j * np.pi * (f + 20.0) * t)
    x0 = x0.astype(np.complex64)  # (one generated block + five rotations of it: the timing does not depend on the content)
    xd = [torch.from_numpy(np.roll(x0, 1009 * i).view(np.float32)).to("cuda") for i in range(6)]
    ctx.set_pipelined(True, 0)
    for i in range(16):
        ctx.push_device(xd[i % 6].data_ptr(), push)
    ctx.sync()
    best = 0.0
    for _trial in range(3):
        t0 = time.perf_counter()
        for i in range(nblocks):
            ctx.push_device(xd[i % 6].data_ptr(), push)
        ctx.sync()
        best = max(best, push * nblocks / (time.perf_counter() - t0) / 1e6)
    ctx.timing_enable(True, families=[ctx.family_index("tick")])
    for i in range(nblocks):
        ctx.push_device(xd[i % 6].data_ptr(), push)
    ctx.sync()
    ms, n = ctx.timing_read()["tick"]
    st = ctx.pipeline_stats()
    ctx.close()
    print(json.dumps({"Msps": round(best, 1), "tick_us": round(ms / max(1, n) * 1e3, 2), "launches": int(n), "pass_blocks": st["pass_blocks"], "depth": st["depth"],
                      "roles": sorted(st["roles"])}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--blocks", type=int, default=60)
    ap.add_argument("--rows", default="0,1,2", help="indices into ROWS")
    ap.add_argument("--out", default=None, help="append the tables (markdown) to this file")
    ap.add_argument("--child", default=None)
    ap.add_argument("--sr", type=float, default=0.0)
    ap.add_argument("--nvfo", type=int, default=0)
    ap.add_argument("--push", type=int, default=0)
    ap.add_argument("--demod", default="CW")
    ap.add_argument("variants", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child(a.sr, a.nvfo, a.push, a.child, a.blocks, a.demod)
    rows = [ROWS[int(i)] for i in a.rows.split(",")]
    res = {}
    for rnd in range(a.rounds):
        for sr, nvfo, push in rows:
            for v in a.variants:
                label, spec = v.split("=", 1)
                parts = spec.split(",")
                opts = dict(kv.split("=", 1) for kv in parts[1:])
                cmd = [sys.executable, os.path.abspath(__file__), "--child", parts[0], "--sr", str(sr), "--nvfo", str(nvfo), "--push", str(push), "--blocks", str(a.blocks),
                       "--demod", opts.get("demod", "CW")]
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                line = [l for l in r.stdout.splitlines() if l.startswith("{")]
                if r.returncode != 0 or not line:
                    print("## %s %.2f MS/s push %d FAILED rc %d: %s" % (label, sr / 1e6, push, r.returncode, (r.stderr or r.stdout)[-600:]), flush=True)
                    return 1  # (nothing more is started on the device behind a failed run)
                o = json.loads(line[-1])
                res.setdefault((sr, nvfo, push), {}).setdefault(label, []).append(o)
                print("round %d  %-10s %6.2f MS/s x %3d VFOs push %8d  %9.1f MS/s  tick %8.2f us  (%d launches, %d ordinary, depth %d)" % (
                    rnd, label, sr / 1e6, nvfo, push, o["Msps"], o["tick_us"], o["launches"], o["pass_blocks"], o["depth"]), flush=True)
    table = []
    labels = [v.split("=", 1)[0] for v in a.variants]
    for (sr, nvfo, push), per in res.items():
        table += ["### %d CW VFOs at %.2f MS/s, blocks of %d samples, pipelined; %d rounds of %d blocks per variant" % (nvfo, sr / 1e6, push, a.rounds, a.blocks), "",
                  "| variant | Msamples/s (median) | min .. max | tick us per block (median) | min .. max | depth | blocks as ordinary passes | first-stage roles |", "|---|---|---|---|---|---|---|---|"]
        med = {}
        for label in labels:
            rs = per[label]
            ms, tk = sorted(x["Msps"] for x in rs), sorted(x["tick_us"] for x in rs)
            med[label] = (tk[len(tk) // 2], tk[-1] - tk[0])
            front = [q for q in rs[0]["roles"] if q.startswith(("s1", "fcl", "fcm", "f2", "rot"))]
            table.append("| %s | %.1f | %.1f .. %.1f | %.2f | %.2f .. %.2f | %d | %d | %s |" % (label, ms[len(ms) // 2], ms[0], ms[-1], tk[len(tk) // 2], tk[0], tk[-1], rs[0]["depth"],
                                                                                          sum(x["pass_blocks"] for x in rs), ", ".join(front)))
        if len(labels) >= 2:
            (ta, spread), (tb, _) = med[labels[0]], med[labels[1]]
            table += ["", "Tick time, %s - %s: %+.2f us per block (%.2fx); run-to-run spread of `%s` (max - min over its rounds): %.2f us — %s." % (
                labels[1], labels[0], tb - ta, ta / tb if tb > 0 else 0.0, labels[0], spread,
                "below the parent by more than its spread" if ta - tb > spread else ("inside the spread" if abs(tb - ta) <= spread else "ABOVE the parent by more than its spread")), ""]
    print("\n".join(table))
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(table) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
