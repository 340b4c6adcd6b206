#!/usr/bin/env python3
"""Host-fed ingest rate of the headline workload (cfg 3) by wire format: float32 sdrpp_push against sdrpp_push_int16 and sdrpp_push_raw with int16, int8 and
table-converted uint8 samples — pipelined, with bench.py's grouping (4 blocks per launch at 10^6-sample blocks, SDRPP_GROUP_MAX at sample_rate / 200, adaptive),
source blocks in page-locked host memory, outputs left on the device (result_flags 0) and with every VFO block + zoomed lines delivered (flags 3).  Next to the
rate: the tick kernel's own duration (HIP events on the launch), i.e. what a converting landing copy costs the launch against the verbatim one.

    tools/ingest_rate.py --rounds 7  f32=push  i16=raw_i16  i8=raw_i8  u8=raw_u8  int16=int16  parent_int16=int16@/path/to/parent/tree

A variant is  label=<method>[@<tree>]: method push | int16 | raw_i16 | raw_i8 | raw_u8, tree = a checkout whose sdrplusplus_amd package (and built library) the
child process imports instead of this one — how sdrpp_push_int16 of the PARENT commit runs in the same call on the same box.  Variants are interleaved round by
round, every run in a process of its own (as tools/ab_tick.py does), so that box drift shows as scatter; the summary gives median and range over the rounds."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM_CAP = 1000000


def child(method, tree, group):
    sys.path.insert(0, tree)
    import numpy as np

    from sdrplusplus_amd import capi, workloads

    sr, nvfo = workloads.CFG[3]["sr"], workloads.CFG[3]["nvfo"]
    out = {}
    for B in (STREAM_CAP, int(sr / 200)):
        G = max(1, min(capi.GROUP_MAX, group if B >= STREAM_CAP else capi.GROUP_MAX))
        ctx = capi.Context(0, max_push=B * G)
        workloads.setup(ctx, 3, dense_fft=True, data_width=1024, nvfo=nvfo)
        if B < STREAM_CAP:
            ctx.set_reference_block(B)
        nb = max(8, 2 * G)
        x0 = workloads.synth(3, B, seed=7, nvfo=nvfo).view(np.float32)  # (one generated block and rotations of it: the timing does not depend on the content)
        bps = {"push": 8, "int16": 4, "raw_i16": 4, "raw_i8": 2, "raw_u8": 2}[method]
        pin = ctx.L.sdrpp_host_alloc(nb * B * bps)
        for i in range(nb):
            x = np.roll(x0, 2 * 1009 * i)
            if bps == 8:
                q = x
            elif bps == 4:
                q = np.clip(np.round(x * 20000.0), -32768, 32767).astype(np.int16)
            else:
                q = np.clip(np.round(x * 100.0), -128, 127).astype(np.int8)
                if method == "raw_u8":
                    q = (q.astype(np.int16) + 128).astype(np.uint8)
            C.memmove(pin + i * B * bps, q.ctypes.data, B * bps)
        L, h = ctx.L, ctx.h
        if method == "push":
            push = lambda i: ctx._chk(L.sdrpp_push(h, C.cast(C.c_void_p(pin + (i % nb) * B * 8), C.POINTER(C.c_float)), B))  # noqa: E731
        elif method == "int16":
            push = lambda i: ctx._chk(L.sdrpp_push_int16(h, C.cast(C.c_void_p(pin + (i % nb) * B * 4), C.POINTER(C.c_int16)), B))  # noqa: E731
        else:
            tab = capi.design_u8_table(capi.U8_RTL_SDR)
            fmt = {"raw_i16": capi.IqFormat(capi.IQ_I16, 32768.0, None), "raw_i8": capi.IqFormat(capi.IQ_I8, 128.0, None),
                   "raw_u8": capi.IqFormat(capi.IQ_U8, 0.0, tab.ctypes.data_as(C.POINTER(C.c_float)))}[method]
            push = lambda i: ctx._chk(L.sdrpp_push_raw(h, C.c_void_p(pin + (i % nb) * B * bps), B, C.byref(fmt)))  # noqa: E731
        npush = max(8, min(400, (1 << 26) // B), 40 * G if B < STREAM_CAP else 0)

        def rate(fn, end):
            for i in range(8):
                fn(i)
            end()
            best = 0.0
            for _trial in range(3):
                t0 = time.perf_counter()
                for i in range(npush):
                    fn(i)
                end()
                best = max(best, B * npush / (time.perf_counter() - t0) / 1e6)
            return round(best, 1)

        e = {}
        ctx.set_pipelined(True, 0)
        ctx.set_pipeline_group(G, True)
        e["no_read_Msps"] = rate(push, ctx.sync)
        ctx.timing_enable(True, families=[ctx.family_index("tick")])
        for i in range(npush):
            push(i)
        ctx.sync()
        ms, n = ctx.timing_read()["tick"]
        ctx.timing_enable(False)
        e["tick_us_per_block"] = round(ms * 1e3 / npush, 2)
        e["tick_us_per_launch"] = round(ms * 1e3 / max(1, n), 2)
        st = ctx.pipeline_stats()
        e["pass_blocks"] = st["pass_blocks"]
        ctx.set_pipeline_group(1, False)
        ctx.set_pipelined(False)
        ctx.set_pipelined(True, 3)
        ctx.set_pipeline_group(G, True)
        lag = min(capi.RESULT_SLOTS - 2, int(st["depth"]) + 2) * G
        state = {"next": ctx.ticket() + 1}

        def collect(upto):
            while state["next"] <= upto:
                t = C.c_uint64(state["next"])
                r = capi.Result()
                ctx._chk(L.sdrpp_result_wait(h, t, C.byref(r)))
                ctx._chk(L.sdrpp_result_release(h, t))
                state["next"] += 1

        def with_results(i):
            push(i)
            collect(ctx.ticket() - lag)

        e["delivered_Msps"] = rate(with_results, lambda: collect(ctx.ticket()))
        e["pass_blocks"] += ctx.pipeline_stats()["pass_blocks"]
        ctx.close()
        L.sdrpp_host_free(pin)
        out[str(B)] = e
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--child", default=None)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("variants", nargs="*")
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.tree, a.group)
    res = {}
    for rnd in range(a.rounds):
        for v in a.variants:
            label, spec = v.split("=", 1)
            method, _, tree = spec.partition("@")
            cmd = [sys.executable, os.path.abspath(__file__), "--child", method, "--tree", os.path.abspath(tree) if tree else ROOT, "--group", str(a.group)]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            except subprocess.TimeoutExpired:
                print("## %s round %d: no result within 300 s; stopping" % (label, rnd), flush=True)
                return 1
            line = [l for l in r.stdout.splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                print("## %s round %d FAILED rc %d: %s" % (label, rnd, r.returncode, (r.stderr or r.stdout)[-800:]), flush=True)
                return 1  # (nothing more is started on the device behind a run that failed)
            o = json.loads(line[-1])
            for B, e in o.items():
                res.setdefault((label, int(B)), []).append(e)
                print("round %d  %-14s push %8s  no read %8.1f MS/s  delivered %8.1f MS/s  tick %8.2f us / block (%8.2f / launch)  ordinary %d" %
                      (rnd, label, B, e["no_read_Msps"], e["delivered_Msps"], e["tick_us_per_block"], e["tick_us_per_launch"], e["pass_blocks"]), flush=True)
    print("---- summary: median [min .. max] over %d rounds ----" % a.rounds)
    print("| variant | push | no read, MS/s | delivered, MS/s | tick, us / block |")
    print("|---|---|---|---|---|")
    for (label, B), rs in sorted(res.items(), key=lambda kv: (-kv[0][1], kv[0][0])):
        def mm(k):
            v = sorted(x[k] for x in rs)
            return "%.1f [%.1f .. %.1f]" % (v[len(v) // 2], v[0], v[-1])
        print("| %s | %d | %s | %s | %s |" % (label, B, mm("no_read_Msps"), mm("delivered_Msps"), mm("tick_us_per_block")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
