#!/usr/bin/env python3
"""The CKKS batch encoder (lr_ckks_encoder) on both routes, timed in the same process.

    python tools/ckks_encoder_bench.py [--sets PN15QP880,PN16QP1761] [--batches 1,32,256] [--reps 5] [--iters 5] [--warmup 2] [--no-python]

Per parameter set, slot count (N / 2 and 2^10) and batch size: Encode and Decode at the top level through the device-pointer entry points
(slot values resident in HBM: the kernels and their launches, nothing else) on the route the slot count takes by itself and, where that is
the fused one, on the tiled route too (lr_options::ckks_encoder_tiled), and the host-value Encode / Decode of the default route (staging
through the pinned buffer and PCIe included).  Every repetition times each leg once, in alternating order, as `iters` back-to-back calls
between two device synchronisations (after `warmup` untimed calls per leg).  Reported: the median and the spread (min, max) over the
repetitions in microseconds per call and the median rate in plaintexts per second.  Next to them, only as orientation, the rate of the
Python restatement (tests/ckks_encoder_ref.py over the CPU oracle) on one plaintext of the same shape.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as graft  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batches", default="1,32,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-python", action="store_true", help="skip the Python restatement's rate")
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    scale = 2.0 ** 40
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call; rate in plaintexts per second", "sets": {}}
    for name in args.sets.split(","):
        N, Q, _ = params.ckks_moduli(name)
        level = len(Q) - 1
        cQ = ring.NewContextWithParams(N, Q)
        per_set = {"N": N, "limbs_q": len(Q), "level": level, "slots": {}}
        for slots in (N // 2, 1 << 10):
            per_slots = {"batches": {}}
            rng = np.random.default_rng(slots)
            if not args.no_python:
                import ckks_encoder_ref as ref
                r = ref.Encoder(graft.load_oracle(), N, Q)
                v = rng.uniform(-1, 1, slots) + 1j * rng.uniform(-1, 1, slots)
                t0 = time.perf_counter()
                pt_ref = r.encode(v, level, scale)
                t1 = time.perf_counter()
                r.decode(pt_ref, slots, level, scale)
                t2 = time.perf_counter()
                per_slots["python_restatement"] = {"encode_rate": round(1 / (t1 - t0), 3), "decode_rate": round(1 / (t2 - t1), 3)}
            for batch in [int(b) for b in args.batches.split(",")]:
                natural = ring.CkksEncoder(cQ, batch)
                encoders = {"fused" if natural.fused(slots) else "tiled": natural}
                if natural.fused(slots):
                    encoders["tiled"] = ring.CkksEncoder(cQ, batch, options=ring.Options(ckks_encoder_tiled=1))
                vals = rng.uniform(-1, 1, (batch, slots)) + 1j * rng.uniform(-1, 1, (batch, slots))
                flat = np.zeros(batch * N, dtype=np.uint64)
                flat[:batch * slots * 2] = vals.view(np.uint64).reshape(-1)
                d_vals = ring.Poly(cQ, 1, batch).set(flat.reshape(batch, 1, N))      # one-limb polys as plain device buffers
                d_out = ring.Poly(cQ, 1, batch)
                pt = cQ.NewPoly(batch)
                legs = {}
                for route, enc in encoders.items():
                    legs["encode_" + route] = (lambda enc=enc: enc.EncodeDevice(pt, d_vals.device_ptr, slots, level, scale, batch))
                    legs["decode_" + route] = (lambda enc=enc: enc.DecodeDevice(pt, slots, level, scale, d_out.device_ptr))
                legs["encode_host_values"] = lambda: natural.Encode(pt, vals, level, scale)
                legs["decode_host_values"] = lambda: natural.Decode(pt, slots, level, scale)
                natural.Encode(pt, vals, level, scale)
                for f in legs.values():
                    for _ in range(args.warmup):
                        f()
                cQ.Sync()
                # both routes, the same bits, at the size that is timed
                if len(encoders) == 2 and batch <= 32:
                    a = encoders["fused"].Encode(cQ.NewPoly(batch), vals, level, scale)
                    b = encoders["tiled"].Encode(cQ.NewPoly(batch), vals, level, scale)
                    assert np.array_equal(a.get(), b.get())
                    assert np.array_equal(encoders["fused"].Decode(a, slots, level, scale).view(np.uint64), encoders["tiled"].Decode(a, slots, level, scale).view(np.uint64))
                    del a, b
                times = {leg: [] for leg in legs}
                order = list(legs)
                for rep in range(args.reps):
                    for leg in (order if rep % 2 == 0 else order[::-1]):
                        f = legs[leg]
                        cQ.Sync()
                        t0 = time.perf_counter()
                        for _ in range(args.iters):
                            f()
                        cQ.Sync()
                        times[leg].append((time.perf_counter() - t0) / args.iters * 1e6)
                out = {}
                for leg, v in times.items():
                    med = statistics.median(v)
                    out[leg] = {"median": round(med, 2), "min": round(min(v), 2), "max": round(max(v), 2), "rate": round(batch / med * 1e6, 1)}
                per_slots["batches"][str(batch)] = out
            per_set["slots"][str(slots)] = per_slots
        result["sets"][name] = per_set
    print(json.dumps(result))


if __name__ == "__main__":
    main()
