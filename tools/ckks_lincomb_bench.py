#!/usr/bin/env python3
"""res = c0 + sum c_k ct_k as one device call (lr_ckks_lincomb), timed in one process beside the sequence it replaces.

    python tools/ckks_lincomb_bench.py [--sets PN15QP880,PN16QP1761] [--batches 1,256] [--terms 2,4,16] [--reps 5] [--iters 2] [--warmup 1]
                                       [--max-gib 96]

Per parameter set at its top level, batch size, term count T and with / without pre-multipliers on every term, distinct ciphertexts
resident in HBM (their contents do not matter to integer kernels: the polys are used as allocated, only the batch-1 shapes are filled):

    fused            Context.CkksLinComb from zero with a constant: (T + 1) * 2 row passes
    parent_sequence  what the overlay's patched AddConst / MultByConstAndAdd did until now, through the mirror: Context.HalfScalarOp "ADD"
                     on component 0, then per term and component "MRED" on the receiver where it has a pre-multiplier and "MRED_ADD"
                     (3 T + 2 to 5 T + 2 row passes; the zeroing of the fresh receiver is not counted)

Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after
`warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call;
`fused_over_parent`, the ratio of the medians, whichever way it comes out; and `fused_fraction_of_roofline`, the time 8 TB/s needs for
the fused call's (T + 1) * 2 row passes over the fused median.  At batch 1 the two legs are checked to give the same bits before they
are timed.  A shape whose polys would take more than --max-gib runs at the largest batch that fits (`batch_used`).  Prints one JSON
object; nothing is gated on it."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402

from ckks_encryptor_bench import time_legs  # noqa: E402

HBM_BYTES_PER_S = 8e12


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--terms", default="2,4,16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--max-gib", type=float, default=96.0)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    if pkg._native.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    rng = np.random.default_rng(1)
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "roofline_bytes_per_s": HBM_BYTES_PER_S, "sets": {}}
    for name in args.sets.split(","):
        N, Q, _ = params.ckks_moduli(name)
        Q = [int(q) for q in Q]
        nQ, level = len(Q), len(Q) - 1
        ctx = ring.NewContextWithParams(N, Q)
        row_bytes = nQ * N * 8
        entry = {"N": N, "limbs": nQ, "level": level, "shapes": []}
        words = lambda: np.array([int(rng.integers(0, q)) for q in Q], dtype=np.uint64)
        for batch in [int(b) for b in args.batches.split(",")]:
            for T in [int(t) for t in args.terms.split(",")]:
                used = max(1, min(batch, int(args.max_gib * 2 ** 30 // ((2 * T + 4) * row_bytes))))
                cts = [(ctx.NewPoly(used), ctx.NewPoly(used)) for _ in range(T)]
                out, out_p = (ctx.NewPoly(used), ctx.NewPoly(used)), (ctx.NewPoly(used), ctx.NewPoly(used))
                if used == 1:
                    for k, ct in enumerate(cts):
                        for u in range(2):
                            ct[u].set(sampling.uniform_poly(Q, N, 1, seed=100 + 2 * k + u))
                add = (words(), words())
                pre, lo, hi = (np.array([words() for _ in range(T)], dtype=np.uint64) for _ in range(3))
                for with_pre in (0, 1):
                    has_pre = np.full(T, with_pre, dtype=np.uint8)
                    consts = ring.CkksLinCombConsts(level, 0.0, add, has_pre, pre, lo, hi)

                    def fused():
                        ctx.CkksLinComb(level, cts, consts, add=add, accumulate=False, out=out)

                    def parent():
                        ctx.HalfScalarOp("ADD", level, out_p[0], add[0], add[1], out_p[0])
                        for k, ct in enumerate(cts):
                            for u in range(2):
                                if with_pre:
                                    ctx.HalfScalarOp("MRED", level, out_p[u], pre[k], pre[k], out_p[u])
                                ctx.HalfScalarOp("MRED_ADD", level, ct[u], lo[k], hi[k], out_p[u])
                    checked = False
                    if used == 1:
                        out_p[0].Zero()
                        out_p[1].Zero()
                        fused()
                        parent()
                        checked = all(np.array_equal(out[u].get(), out_p[u].get()) for u in range(2))
                        if not checked:
                            raise SystemExit("the legs disagree at %s batch %d T %d" % (name, used, T))
                    times = time_legs({"fused": fused, "parent_sequence": parent}, ctx.Sync, args.reps, args.iters, args.warmup)
                    o = {"batch": batch, "batch_used": used, "terms": T, "pre_multipliers": bool(with_pre), "bit_exact_between_legs": checked if used == 1 else None}
                    o.update({leg: summarise(v) for leg, v in times.items()})
                    o["fused_over_parent"] = round(o["fused"]["median"] / o["parent_sequence"]["median"], 3)
                    roof_us = (T + 1) * 2 * used * row_bytes / HBM_BYTES_PER_S * 1e6
                    o["fused_fraction_of_roofline"] = round(roof_us / o["fused"]["median"], 3)
                    entry["shapes"].append(o)
                del cts, out, out_p
        result["sets"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
