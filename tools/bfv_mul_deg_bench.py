#!/usr/bin/env python3
"""BFV Mul for every operand degree (lr_bfv_mul_deg) against the degree-1 x degree-1 product (lr_bfv_mul), timed in the same process.

    python tools/bfv_mul_deg_bench.py [--set PN14QP438] [--batches 1,256] [--reps 7] [--iters 20] [--warmup 5]

Shapes: (1,1) through lr_bfv_mul, (1,0) = ciphertext x plaintext, (2,1) = a degree-2 result times a ciphertext, (2,2) squaring.  Every
repetition times each shape once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after `warmup`
untimed calls per shape); the line reports the median and the spread (min, max) over the repetitions, in microseconds per call, and each
shape's median relative to lr_bfv_mul's at the same batch.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import __graft_entry__ as graft  # noqa: E402

SHAPES = [("1x1_mul", 1, 1, False), ("1x0_ct_pt", 1, 0, False), ("2x1", 2, 1, False), ("2x2_square", 2, 2, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--set", default="PN14QP438")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    N, Q, _, QMul = params.bfv_moduli(args.set)
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)
    result = {"set": args.set, "N": N, "limbs_q": len(Q), "limbs_qmul": len(QMul), "reps": args.reps, "iters": args.iters,
              "warmup": args.warmup, "unit": "us per call", "batches": {}}
    for batch in [int(b) for b in args.batches.split(",")]:
        plan = ring.BfvPlan(cQ, cM, 65537, batch)
        polys = [cQ.NewPoly(batch).set(sampling.uniform_poly(Q, N, batch, seed=90 + k).reshape(batch, len(Q), N)) for k in range(6)]
        outs = [cQ.NewPoly(batch) for _ in range(5)]
        calls = {}
        for name, d0, d1, sq in SHAPES:
            ct0 = polys[:d0 + 1]
            ct1 = ct0 if sq else polys[3:3 + d1 + 1]
            out = outs[:d0 + d1 + 1]
            if (d0, d1) == (1, 1):
                calls[name] = (lambda ct0=ct0, ct1=ct1, out=out: plan.Mul(ct0, ct1, out))
            else:
                calls[name] = (lambda ct0=ct0, ct1=ct1, out=out: plan.MulDeg(ct0, ct1, out))
        for f in calls.values():
            for _ in range(args.warmup):
                f()
        cQ.Sync()
        times = {name: [] for name in calls}
        order = list(calls)
        for rep in range(args.reps):
            for name in (order if rep % 2 == 0 else order[::-1]):
                f = calls[name]
                cQ.Sync()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    f()
                cQ.Sync()
                times[name].append((time.perf_counter() - t0) / args.iters * 1e6)
        base = statistics.median(times["1x1_mul"])
        result["batches"][str(batch)] = {
            name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                   "vs_mul": round(statistics.median(v) / base, 3)} for name, v in times.items()}
    print(json.dumps(result))


if __name__ == "__main__":
    main()
