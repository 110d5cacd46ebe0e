#!/usr/bin/env python3
"""CKKS Add / Sub of any scale, level and degree as one device call (lr_ckks_combine), timed in one process beside the sequence it
replaces.

    python tools/ckks_combine_bench.py [--sets PN15QP880,PN16QP1761] [--batches 1,256] [--reps 5] [--iters 2] [--warmup 1] [--max-gib 96]

Per parameter set at its top level and batch size, distinct ciphertexts resident in HBM (their contents do not matter to integer kernels:
the polys are used as allocated, only the batch-1 shapes are filled), four calls:

    add              Add of two degree-1 ciphertexts of equal scales into a third.  Sequence: AddLvl per component (6 row passes; the
                     fused call moves the same 6)
    add_equalised    the same with unequal scales: MultByConst of b into the pool ciphertext, then AddLvl.  Sequence: HalfScalarOp
                     "MRED" and AddLvl per component (10 row passes; fused 6)
    chebyshev_step   C[n] = 2 C[n] - r C[c] in place, C[n] of the smaller scale: Add(C[n], C[n], C[n]), MultByConst in place, Sub.
                     Sequence: AddLvl, HalfScalarOp "MRED" and SubLvl per component (14 row passes; fused 6)
    sub_deg2_deg1    Sub of a degree-1 from a degree-2 ciphertext into a third.  Sequence: SubLvl on two components, CopyLvl on the
                     third (8 row passes; fused 8)

Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after
`warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call;
`fused_over_parent`, the ratio of the medians, whichever way it comes out; and `fused_fraction_of_roofline`, the time 8 TB/s needs for
the fused call's row passes over the fused median.  At batch 1 the two legs are checked to give the same bits before they are timed.  A
shape whose polys would take more than --max-gib runs at the largest batch that fits (`batch_used`).  Prints one JSON object; nothing is
gated on it."""
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
POLYS = 18          # what one shape holds: a (degree 2) and b (degree 1) and a receiver of three components per leg, and the pool


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batches", default="1,256")
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
        mult = np.array([int(rng.integers(0, q)) for q in Q], dtype=np.uint64)
        for batch in [int(b) for b in args.batches.split(",")]:
            used = max(1, min(batch, int(args.max_gib * 2 ** 30 // (POLYS * row_bytes))))
            new = lambda n: [ctx.NewPoly(used) for _ in range(n)]
            # a (degree 2) and b (degree 1) once per leg, because the Chebyshev step writes its first operand; a receiver per leg; the pool
            a_f, a_p, b_f, b_p, out_f, out_p, pool = new(3), new(3), new(2), new(2), new(3), new(3), new(2)

            def fill():
                if used == 1:
                    for u in range(3):
                        d = sampling.uniform_poly(Q, N, 1, seed=100 + u)
                        a_f[u].set(d), a_p[u].set(d)
                    for u in range(2):
                        d = sampling.uniform_poly(Q, N, 1, seed=200 + u)
                        b_f[u].set(d), b_p[u].set(d)

            def seq_add():
                for u in range(2):
                    ctx.AddLvl(level, a_p[u], b_p[u], out_p[u])

            def seq_add_equalised():
                for u in range(2):
                    ctx.HalfScalarOp("MRED", level, b_p[u], mult, mult, pool[u])
                for u in range(2):
                    ctx.AddLvl(level, a_p[u], pool[u], out_p[u])

            def seq_chebyshev():
                for u in range(2):
                    ctx.AddLvl(level, a_p[u], a_p[u], a_p[u])
                for u in range(2):
                    ctx.HalfScalarOp("MRED", level, a_p[u], mult, mult, a_p[u])
                for u in range(2):
                    ctx.SubLvl(level, a_p[u], b_p[u], a_p[u])

            def seq_sub21():
                for u in range(2):
                    ctx.SubLvl(level, a_p[u], b_p[u], out_p[u])
                ctx.CopyLvl(level, a_p[2], out_p[2])

            calls = [
                ("add", lambda: ctx.CkksCombine("ADD", level, a_f[:2], b_f, out_f[:2]), seq_add, 6, lambda: (out_f[:2], out_p[:2])),
                ("add_equalised", lambda: ctx.CkksCombine("ADD", level, a_f[:2], b_f, out_f[:2], mb=mult), seq_add_equalised, 6, lambda: (out_f[:2], out_p[:2])),
                ("chebyshev_step", lambda: ctx.CkksCombine("SUB", level, a_f[:2], b_f, a_f[:2], double_a=True, ma=mult), seq_chebyshev, 6,
                 lambda: (a_f[:2], a_p[:2])),
                ("sub_deg2_deg1", lambda: ctx.CkksCombine("SUB", level, a_f, b_f, out_f), seq_sub21, 8, lambda: (out_f, out_p)),
            ]
            for call, fused, parent, passes, results in calls:
                checked = None
                if used == 1:
                    fill()
                    fused()
                    parent()
                    got, want = results()
                    checked = all(np.array_equal(g.get(), w.get()) for g, w in zip(got, want))
                    if not checked:
                        raise SystemExit("the legs disagree at %s batch %d %s" % (name, used, call))
                times = time_legs({"fused": fused, "parent_sequence": parent}, ctx.Sync, args.reps, args.iters, args.warmup)
                o = {"call": call, "batch": batch, "batch_used": used, "fused_row_passes": passes, "bit_exact_between_legs": checked}
                o.update({leg: summarise(v) for leg, v in times.items()})
                o["fused_over_parent"] = round(o["fused"]["median"] / o["parent_sequence"]["median"], 3)
                roof_us = passes * used * row_bytes / HBM_BYTES_PER_S * 1e6
                o["fused_fraction_of_roofline"] = round(roof_us / o["fused"]["median"], 3)
                entry["shapes"].append(o)
            del a_f, a_p, b_f, b_p, out_f, out_p, pool
        result["sets"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
