#!/usr/bin/env python3
"""BFV Relinearize of a degree-3..5 ciphertext as one device call (lr_bfv_relinearize_deg), timed in one process beside the composed route
and beside the host loop it replaces.

    python tools/bfv_relin_deg_bench.py [--sets PN13QP218,PN14QP438] [--degrees 3,5] [--batches 1,8,64] [--max-batch 256]
                                        [--rounds 3] [--reps 5] [--iters 4] [--warmup 2]

Per parameter set, degree and batch size, uniform ciphertexts and keys resident in HBM, one different key per degree, every plan made
with `--max-batch`:

    relin_deg               the call on a default plan: its default route
    relin_deg_composed      the call on a plan made with lr_options::no_epilogue over default contexts: the composed route -- per degree the
                            key switch and the two Adds -- with the very kernels of the default plan's key switch; the leg the route decision
                            compares against
    relin_deg_no_epilogue   the call where the contexts carry no_epilogue as well: the composed route with the call-by-call ModDown
    host_loop               what the overlay did until now, through the mirror: two Context.Copy, then per degree CkksPlan.BfvSwitchKeys and
                            two Context.Add

A round times each leg `reps` times in alternating order, each time as `iters` back-to-back calls between two synchronisations of the
stream (after `warmup` untimed calls per leg), and takes the median per leg.  `rounds` rounds give repeated medians: reported per leg are
these medians, their median and their spread (max - min) in microseconds per call.  `merged_not_slower`: the default route's median is
within the composed leg's by no more than the larger of the two legs' spreads.  Before the timing the four legs are checked to give the
same bits.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

from ckks_encryptor_bench import time_legs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN13QP218,PN14QP438")
    ap.add_argument("--degrees", default="3,5")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--max-batch", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    if pkg._native.device_count() < 1:
        raise SystemExit("no HIP device: nothing here is measured on a CPU")
    result = {"max_batch": args.max_batch, "rounds": args.rounds, "reps": args.reps, "iters": args.iters, "warmup": args.warmup,
              "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.bfv_moduli(name)[:3]
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        beta = -(-len(Q) // len(P))
        keys_h = [sampling.uniform_poly(Q + P, N, 2 * beta, seed=800 + i) for i in range(4)]
        entry = {"N": N, "limbs_q": len(Q), "limbs_p": len(P), "beta": beta, "cases": {}}
        for degree in [int(d) for d in args.degrees.split(",")]:
            for batch in [int(b) for b in args.batches.split(",")]:
                ct_h = [np.tile(sampling.uniform_poly(Q, N, 1, seed=900 + k), (batch, 1, 1)) for k in range(degree + 1)]
                plans = {}
                for shape, ctx_opt, plan_opt in (("default", ring.Options(), ring.Options()), ("composed", ring.Options(), ring.Options(no_epilogue=1)),
                                                 ("no_epilogue", ring.Options(no_epilogue=1), ring.Options(no_epilogue=1))):
                    cQ, cP = ring.NewContextWithParams(N, Q, options=ctx_opt), ring.NewContextWithParams(N, P, options=ctx_opt)
                    plan = ring.CkksPlan(cQ, cP, args.max_batch, options=plan_opt)
                    keys = [plan.NewSwitchingKey().set(k) for k in keys_h[:degree - 1]]
                    ct = [cQ.NewPoly(batch).set(x) for x in ct_h]
                    plans[shape] = (cQ, cP, plan, keys, ct, (cQ.NewPoly(batch), cQ.NewPoly(batch)))
                cQ, cP, plan, keys, ct, out = plans["default"]
                acc, pool = (cQ.NewPoly(batch), cQ.NewPoly(batch)), (cQ.NewPoly(batch), cQ.NewPoly(batch))

                def host_loop():
                    cQ.Copy(ct[0], acc[0])                                              # bfv/evaluator.go:484-487
                    cQ.Copy(ct[1], acc[1])
                    for deg in range(degree, 1, -1):
                        plan.BfvSwitchKeys(ct[deg], keys[deg - 2], pool[0], pool[1])    # :493
                        cQ.Add(acc[0], pool[0], acc[0])                                 # :494
                        cQ.Add(acc[1], pool[1], acc[1])                                 # :495

                def call(shape):
                    _, _, pl, ks, c, o = plans[shape]
                    return lambda: pl.BfvRelinearizeDeg(c, ks, o)
                legs = {"relin_deg": call("default"), "relin_deg_composed": call("composed"), "relin_deg_no_epilogue": call("no_epilogue"),
                        "host_loop": host_loop}

                def sync_all():
                    for p in plans.values():
                        p[1].Sync()
                        p[0].Sync()
                for f in legs.values():
                    f()
                sync_all()
                want = [p.get() for p in out]
                for got in [plans["composed"][5], plans["no_epilogue"][5], acc]:
                    if not all(np.array_equal(got[k].get(), want[k]) for k in range(2)):
                        raise SystemExit("the legs disagree at %s degree %d batch %d" % (name, degree, batch))
                medians = {leg: [] for leg in legs}
                for _ in range(args.rounds):
                    times = time_legs(legs, sync_all, args.reps, args.iters, args.warmup)
                    for leg, v in times.items():
                        medians[leg].append(round(statistics.median(v), 1))
                o = {leg: {"medians": m, "median": round(statistics.median(m), 1), "spread": round(max(m) - min(m), 1)} for leg, m in medians.items()}
                slack = max(o["relin_deg"]["spread"], o["relin_deg_composed"]["spread"])
                o["relin_deg_over_composed"] = round(o["relin_deg"]["median"] / o["relin_deg_composed"]["median"], 3)
                o["relin_deg_over_host_loop"] = round(o["relin_deg"]["median"] / o["host_loop"]["median"], 3)
                o["merged_not_slower"] = bool(o["relin_deg"]["median"] <= o["relin_deg_composed"]["median"] + slack)
                o["groups_per_pass"] = min(degree - 1, max(1, args.max_batch // batch))
                o["bit_exact_between_legs"] = True
                entry["cases"]["degree%d_batch%d" % (degree, batch)] = o
                del plans, legs
        result["sets"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
