#!/usr/bin/env python3
"""What the radio's IF chain costs (sdrpp_vfo_set_if): cfg 4's bank (128 mixed NFM / AM / USB VFOs at 61.44 MS/s) pipelined, blocks read in place in
device memory and left on the device, without a chain, with the squelch on every VFO, and with blanker + squelch on every VFO.  Prints one JSON object
per block size: ingest rate (MS/s, best of three trials) and the time per block (us), plus the one-wavefront-per-VFO figure the tracker is bound by —
IF samples per second and VFO through the chain's role — from a single 250 kS/s RAW VFO at 10^6-sample blocks.
    python tools/ifchain_rate.py [block sizes ...]            (default: 307200 1000000)
    python tools/ifchain_rate.py --fmif [block sizes ...]     FMIF (sdrpp_vfo_set_fmnr) instead: a 32-VFO WFM bank at 10 MS/s, as it is and with 32-bin FMIF on
                                                              every VFO (default sizes: 1000000 50000 = sr / 200) -> profiles/fmif_rate.md"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def rate(ctx, bufs, B, n):
    for i in range(8):
        ctx.push_device(bufs[i % len(bufs)].data_ptr(), B)
    ctx.sync()
    best = 1e30
    for _trial in range(3):
        t0 = time.perf_counter()
        for i in range(n):
            ctx.push_device(bufs[i % len(bufs)].data_ptr(), B)
        ctx.sync()
        best = min(best, (time.perf_counter() - t0) / n)
    return best


def fmif_main(sizes):
    import torch

    from sdrplusplus_amd import capi, radio, workloads

    dev = torch.device("cuda", 0)
    sr, nv = workloads.CFG[3]["sr"], 32
    for B in sizes or [1000000, int(sr / 200)]:
        xs = [workloads.synth(3, B, seed=7 + i, nvfo=nv) for i in range(3)]
        xd = [torch.from_numpy(x.view(np.float32)).to(dev) for x in xs]
        out = {"cfg": 3, "push": B, "nvfo": nv}
        npush = max(24, min(400, (1 << 27) // B))
        for name, bins in (("no_fmif", 0), ("fmif_32", 32), ("fmif_9", 9)):
            ctx = capi.Context(0, max_push=B)
            vids = []
            for mode, if_rate, bw, centre, _ in workloads.vfo_plan(3, nv):
                d, keep = radio.vfo_desc(sr, if_rate, bw, centre, mode)
                vids.append(ctx.vfo_add(d, keep))
                if bins:
                    ctx.vfo_set_fmnr(vids[-1], True, bins)
            ctx.set_pipelined(True, 0)
            dt = rate(ctx, xd, B, npush)
            st = ctx.pipeline_stats()
            assert st["pass_blocks"] == 0, st
            assert (st["roles"].get("ifc", 0) > 0) == bool(bins), st["roles"]
            out[name] = {"MS_per_s": round(B / dt / 1e6, 1), "us_per_block": round(dt * 1e6, 1)}
            ctx.close()
        print(json.dumps(out), flush=True)


def main():
    if "--fmif" in sys.argv[1:]:
        return fmif_main([int(a) for a in sys.argv[1:] if a != "--fmif"])
    import torch

    from sdrplusplus_amd import capi, radio, workloads

    sizes = [int(a) for a in sys.argv[1:]] or [307200, 1000000]
    dev = torch.device("cuda", 0)
    for B in sizes:
        xs = [workloads.synth(4, B, seed=7 + i) for i in range(3)]
        xd = [torch.from_numpy(x.view(np.float32)).to(dev) for x in xs]
        out = {"cfg": 4, "push": B, "nvfo": workloads.CFG[4]["nvfo"]}
        npush = max(24, min(400, (1 << 27) // B))
        for name, nb, sq in (("no_chain", False, None), ("squelch", False, -40.0), ("blanker_squelch", True, -40.0)):
            ctx = capi.Context(0, max_push=B)
            info = workloads.setup(ctx, 4, fft=False)
            if name != "no_chain":
                for vid, (_, if_rate, _, _, _) in zip(info["vids"], info["plan"]):
                    ctx.vfo_set_if(vid, radio.if_desc(if_rate, nb=nb, squelch=sq))
            ctx.set_pipelined(True, 0)
            dt = rate(ctx, xd, B, npush)
            st = ctx.pipeline_stats()
            assert st["pass_blocks"] == 0, st
            assert (st["roles"].get("ifc", 0) > 0) == (name != "no_chain"), st["roles"]
            out[name] = {"MS_per_s": round(B / dt / 1e6, 1), "us_per_block": round(dt * 1e6, 1)}
            ctx.close()
        print(json.dumps(out), flush=True)
    # the tracker's own bound: one wavefront walks one VFO's whole block
    B, sr = 1000000, 1e6
    x = workloads.tones_and_noise(B, sr, 3).astype(np.complex64)
    xd = [torch.from_numpy(x.view(np.float32)).to(dev)]
    one = {}
    for name, f in (("no_chain", None), ("squelch", radio.if_desc(250e3, squelch=-60.0)), ("blanker_squelch", radio.if_desc(250e3, nb=True, squelch=-60.0))):
        ctx = capi.Context(0, max_push=B)
        d, keep = radio.vfo_desc(sr, 250e3, 250e3, 0.0, "RAW")
        vid = ctx.vfo_add(d, keep)
        if f is not None:
            ctx.vfo_set_if(vid, f)
        one[name] = rate(ctx, xd, B, 50)
        ctx.close()
    res = {"if_samples_per_block": B // 4, "us_per_block_no_chain": round(one["no_chain"] * 1e6, 1)}
    for name in ("squelch", "blanker_squelch"):
        extra = one[name] - one["no_chain"]
        res[name] = {"us_per_block": round(one[name] * 1e6, 1), "chain_M_if_samples_per_s": round((B // 4) / max(extra, 1e-9) / 1e6, 1)}
    print(json.dumps({"single_vfo_250k_if": res}), flush=True)


if __name__ == "__main__":
    main()
