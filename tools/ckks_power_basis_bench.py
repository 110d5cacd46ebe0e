#!/usr/bin/env python3
"""The CKKS power basis as one device call (lr_ckks_power_basis), timed in one process beside the composed sequence it stands for.

    python tools/ckks_power_basis_bench.py [--sets PN15QP880,PN16QP1761] [--batches 1,8,32] [--max-batch 32] [--reps 5] [--iters 1]
                                           [--warmup 1] [--out profiles/rNN/ckks_power_basis_bench.json]

Per parameter set at its top level and default scale, per target list -- the Chebyshev lists of EvaluateChebyFast for degrees 9, 33 and
129 and the monomial list of EvaluatePolyFast for degree 33 -- and per batch size, on ONE plan of --max-batch, uniform ciphertexts and
one key image resident in HBM:

    one_call        lr_ckks_power_basis (CkksPlan.PowerBasis): where the plan takes the merged route, chunks of max_batch / batch products
    composed        the sequence it replaces, from the host: per product CkksPlan.MulRelin at mul_level, CkksPlan.Rescale n_rescales
                    times, Context.CkksCombine for the Chebyshev tail

Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after
`warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call, and
the ratio of the medians, whichever way it comes out.  Before the timing the two legs are checked to give the same bits (every product up to batch 8, beyond it the last one).  Prints one JSON
object, and writes it to --out when given."""
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

DEFAULT_SCALE = {"PN12QP109": 2.0 ** 32, "PN13QP218": 2.0 ** 30, "PN14QP438": 2.0 ** 34, "PN15QP880": 2.0 ** 40, "PN16QP1761": 2.0 ** 45}
LISTS = [("cheby_fast_9", 1, 9), ("cheby_fast_33", 1, 33), ("cheby_fast_129", 1, 129), ("poly_fast_33", 0, 33)]


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--max-batch", type=int, default=32)
    ap.add_argument("--lists", default=",".join(n for n, _, _ in LISTS))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    lib, check = pkg._native.lib(), pkg._native.check
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "max_batch": args.max_batch, "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.ckks_moduli(name)
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        nQ, level, delta = len(Q), len(Q) - 1, DEFAULT_SCALE[name]
        beta = -(-nQ // len(P))
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
        plan = ring.CkksPlan(cQ, cP, args.max_batch)
        key = plan.NewSwitchingKey().set(sampling.uniform_poly(Q + P, N, 2 * beta, seed=500))
        ct1 = [np.asarray(sampling.uniform_poly(Q, N, 1, seed=600 + k)).reshape(1, nQ, N) for k in range(2)]
        entry = {"N": N, "limbs_q": nQ, "limbs_p": len(P), "beta": beta, "lists": {}}
        for list_name, chebyshev, degree in LISTS:
            if list_name not in args.lists.split(","):
                continue
            sched = ring.ckks_power_basis_schedule(Q, delta, chebyshev, level, delta, ring.ckks_power_basis_targets(degree, True))
            layers = {}
            for p in sched.products:
                layers[p.layer] = layers.get(p.layer, 0) + 1
            at_list = {"products": len(sched.products), "widest_layer": max(layers.values()), "batches": {}}
            for batch in [int(b) for b in args.batches.split(",")]:
                c1 = tuple(cQ.NewPoly(batch).set(np.tile(c, (batch, 1, 1))) for c in ct1)
                outs = [(cQ.NewPolyLvl(p.level_after, batch), cQ.NewPolyLvl(p.level_after, batch)) for p in sched.products]
                seq = [(cQ.NewPolyLvl(p.mul_level, batch), cQ.NewPolyLvl(p.mul_level, batch)) for p in sched.products]

                def composed():
                    Cn = {1: c1}
                    for k, p in enumerate(sched.products):
                        t = seq[k]
                        for x in t:
                            check(lib.lr_poly_set_limbs(x.h, p.mul_level + 1))
                        plan.MulRelin(p.mul_level, Cn[int(p.a)], Cn[int(p.b)], key, t)
                        for _ in range(p.n_rescales):
                            plan.Rescale(t)
                        L1 = p.level_after + 1
                        if p.tail == 1:
                            m = sched.mult[k][:L1]
                            cQ.CkksCombine("SUB", p.level_after, t, c1, t, double_a=True, ma=m if p.mult_side == 1 else None,
                                           mb=m if p.mult_side == 2 else None)
                        elif p.tail == 2:
                            cQ.CkksCombine("SUB", p.level_after, t, None, t, double_a=True, add=(sched.add[k][:L1], sched.add[k][:L1]))
                        Cn[int(p.n)] = t
                legs = {"one_call": lambda: plan.PowerBasis(level, c1, sched, key, outs), "composed": composed}

                def sync_all():
                    cP.Sync()
                    cQ.Sync()
                # the legs agree before they are timed
                for f in legs.values():
                    f()
                for k, p in enumerate(sched.products):
                    if batch > 8 and k + 1 < len(sched.products):
                        continue                                   # (a large batch: the last product, which hangs on all the others' layers)
                    for u in range(2):
                        if not np.array_equal(outs[k][u].get(), seq[k][u].get()):
                            raise SystemExit("the legs disagree at %s %s batch %d, C[%d]" % (name, list_name, batch, p.n))
                times = time_legs(legs, sync_all, args.reps, args.iters, args.warmup)
                o = {leg: summarise(v) for leg, v in times.items()}
                o["one_call_over_composed"] = round(o["one_call"]["median"] / o["composed"]["median"], 3)
                o["bit_exact_between_legs"] = True
                at_list["batches"][str(batch)] = o
                print("# %s %s batch %d: %s" % (name, list_name, batch, json.dumps(o)), file=sys.stderr, flush=True)
                del c1, outs, seq, legs
            entry["lists"][list_name] = at_list
        result["sets"][name] = entry
        del plan, key, cQ, cP
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
