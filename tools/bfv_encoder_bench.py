#!/usr/bin/env python3
"""The BFV batch encoder (lr_bfv_encoder) on both routes, timed in the same process.

    python tools/bfv_encoder_bench.py [--set PN14QP438] [--t 65537] [--batches 256,1] [--reps 7] [--iters 20] [--warmup 5]

Per batch size: Encode and Decode through the device-pointer entry points (slots resident in HBM: the kernels and their launches, nothing
else) on the fused route and on the composed one (lr_options::bfv_encoder_unfused), the host-value EncodeUint / DecodeUint of the default
route (staging through the pinned buffer and PCIe included), and, as the reference point, Context.InvNTT on a one-limb poly over (N, [t])
of the same batch -- the transform the composed encode contains.  Every repetition times each leg once, in alternating order, as `iters`
back-to-back calls between two device synchronisations (after `warmup` untimed calls per leg).  Reported: the median and the spread (min,
max) over the repetitions in microseconds per call, the median per plaintext, and the share of the HBM roofline of the leg's compulsory
traffic at 8 TB/s -- the |Q| N 8 bytes of a plaintext written by encode (`write_roofline`), read by decode (`read_roofline`).  Prints
one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as graft  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="PN14QP438")
    ap.add_argument("--t", type=int, default=65537)
    ap.add_argument("--batches", default="256,1")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    N, Q, _, _ = params.bfv_moduli(args.set)
    t = args.t
    cQ, cT = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, [t])
    result = {"set": args.set, "N": N, "limbs_q": len(Q), "t": t, "reps": args.reps, "iters": args.iters, "warmup": args.warmup,
              "unit": "us per call", "hbm_bytes_per_s": HBM_BYTES_PER_S, "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        encoders = {"fused": ring.BfvEncoder(cQ, t, batch), "composed": ring.BfvEncoder(cQ, t, batch, options=ring.Options(bfv_encoder_unfused=1))}
        assert encoders["fused"].fused() and not encoders["composed"].fused()
        slots = np.random.default_rng(5).integers(0, t, size=(batch, N), dtype=np.uint64)
        d_slots = ring.Poly(cQ, 1, batch).set(slots.reshape(batch, 1, N))      # one-limb polys as plain device buffers of [batch][N] words
        d_out = ring.Poly(cQ, 1, batch)
        pt = cQ.NewPoly(batch)
        row = cT.NewPoly(batch).set(slots.reshape(batch, 1, N))
        legs = {}
        for route, enc in encoders.items():
            legs["encode_" + route] = (lambda enc=enc: enc.EncodeDevice(d_slots.device_ptr, N, batch, False, pt))
            legs["decode_" + route] = (lambda enc=enc: enc.DecodeDevice(pt, False, d_out.device_ptr))
        legs["encode_host_values"] = lambda: encoders["fused"].EncodeUint(slots, pt)
        legs["decode_host_values"] = lambda: encoders["fused"].DecodeUint(pt)
        legs["invntt_t_one_limb"] = lambda: cT.InvNTT(row, row)
        encoders["fused"].EncodeUint(slots, pt)
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        cQ.Sync()
        # both routes, the same bits, at the size that is timed
        a = encoders["fused"].EncodeUint(slots, cQ.NewPoly(batch)).get()
        b = encoders["composed"].EncodeUint(slots, cQ.NewPoly(batch)).get()
        assert np.array_equal(a, b) and np.array_equal(encoders["composed"].DecodeUint(pt), slots)
        times = {name: [] for name in legs}
        order = list(legs)
        for rep in range(args.reps):
            for name in (order if rep % 2 == 0 else order[::-1]):
                f = legs[name]
                cQ.Sync()
                cT.Sync()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    f()
                cQ.Sync()
                cT.Sync()
                times[name].append((time.perf_counter() - t0) / args.iters * 1e6)
        floor_us = len(Q) * N * 8 * batch / HBM_BYTES_PER_S * 1e6
        out = {}
        for name, v in times.items():
            med = statistics.median(v)
            out[name] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "per_plaintext": round(med / batch, 3)}
            if name.startswith("encode_") and "host" not in name:
                out[name]["write_roofline"] = round(floor_us / med, 4)
            if name.startswith("decode_") and "host" not in name:
                out[name]["read_roofline"] = round(floor_us / med, 4)
        result["batches"][str(batch)] = out
    print(json.dumps(result))


if __name__ == "__main__":
    main()
