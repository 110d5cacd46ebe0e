#!/usr/bin/env python3
"""CKKS rotation chains as one device call (lr_ckks_rotate_chain), timed in one process beside the composed route and beside the host-side
sequences they replace.

    python tools/ckks_chain_bench.py [--sets PN15QP880,PN16QP1761] [--batches 1,256] [--low-level 3] [--reps 5] [--iters 1] [--warmup 1]
                                     [--out profiles/rNN/ckks_chain_bench.json]

Per parameter set, level (the top one and --low-level) and batch size, uniform ciphertexts and keys resident in HBM, one key image per
step (the images hold the same uniform words: what is timed does not depend on them):

    replace                 lr_ckks_rotate_chain, the replacing chain of rotateColumnsPow2 for k = N/2 - 1 (every bit set: log2(N) - 1 steps)
    replace_composed        the same call on a plan and contexts made with lr_options::no_epilogue: lr_ckks_rotate's body per step
    replace_host_loop       the sequence it replaces: CkksPlan.RotateColumnsPow2, a host loop of PermuteNTT calls (and its two copies)
    slot_sum                lr_ckks_rotate_chain, accumulating over 5^(2^i), i = 0 .. log2(N) - 2
    slot_sum_composed       the same on the no_epilogue plan: per step lr_ckks_rotate's body and two Adds
    slot_sum_host_loop      the sequence it replaces: per step CkksPlan.PermuteNTT into a temporary and Context.AddLvl on both components

Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after
`warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call, and
the ratios of the medians, whichever way they come out.  Before the timing the three legs of each chain are checked to give the same bits.
Prints one JSON object, and writes it to --out when given.  The two plans of a batch are resident together with their digit pools: at
PN16QP1761 and 256 ciphertexts that is an estimated 250 GB (9 digits of 4.6 GB each per plan alone), which was not attempted: that set is
run with --batches 1,64 (profiles/r12/ckks_chain_bench.json is the two runs merged)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402

from ckks_encryptor_bench import time_legs  # noqa: E402


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--low-level", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    import ckks_chain_ref
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.ckks_moduli(name)
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        nQ, logn = len(Q), N.bit_length() - 1
        beta = -(-nQ // len(P))
        key_h = sampling.uniform_poly(Q + P, N, 2 * beta, seed=500)
        gens = ckks_chain_ref.slot_sum_elements(N)                                   # log2(N) - 1 elements: the rotations by 2^i to the left
        k_all = (N >> 1) - 1
        assert [g for g, _ in ckks_chain_ref.pow2_steps(N, k_all)] == gens
        entry = {"N": N, "limbs_q": nQ, "limbs_p": len(P), "beta": beta, "steps": len(gens), "levels": {}}
        ct1 = [np.asarray(sampling.uniform_poly(Q, N, 1, seed=600 + k)).reshape(1, nQ, N) for k in range(2)]
        # the contexts and the key images of the two routes serve every level and batch of the set
        rings = {}
        for shape in ("default", "no_epilogue"):
            opt = ring.Options(no_epilogue=1) if shape == "no_epilogue" else ring.Options()
            cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
            rings[shape] = (opt, cQ, cP, [ring.Poly(cQ, nQ + len(P), 2 * beta).set(key_h) for _ in gens])
        for level in sorted({nQ - 1, min(args.low_level, nQ - 1)}, reverse=True):
            at_level = {}
            for batch in [int(b) for b in args.batches.split(",")]:
                ct_h = [np.tile(c[:, :level + 1], (batch, 1, 1)) for c in ct1]
                shapes = {}
                for shape in ("default", "no_epilogue"):
                    opt, cQ, cP, keys = rings[shape]
                    plan = ring.CkksPlan(cQ, cP, batch, options=opt)
                    ct = tuple(cQ.NewPolyLvl(level, batch).set(h) for h in ct_h)
                    out = tuple(cQ.NewPolyLvl(level, batch) for _ in range(2))
                    shapes[shape] = (cQ, cP, plan, keys, ct, out)
                del ct_h
                cQ, cP, plan, keys, ct, out = shapes["default"]
                _, _, plan_n, keys_n, ct_n, out_n = shapes["no_epilogue"]
                acc = tuple(cQ.NewPolyLvl(level, batch) for _ in range(2))
                tmp = tuple(cQ.NewPolyLvl(level, batch) for _ in range(2))
                pow2 = {1 << i: (g, key) for i, (g, key) in enumerate(zip(gens, keys))}

                def slot_sum_host_loop():
                    cQ.CopyLvl(level, ct[0], acc[0])
                    cQ.CopyLvl(level, ct[1], acc[1])
                    for g, key in zip(gens, keys):
                        plan.PermuteNTT(level, acc, g, key, tmp)             # RotateColumns(ct, 2^i, tmp)
                        cQ.AddLvl(level, acc[0], tmp[0], acc[0])             # Add(ct, tmp, ct)
                        cQ.AddLvl(level, acc[1], tmp[1], acc[1])
                legs = {
                    "replace": lambda: plan.RotateChain(level, ct, gens, keys, False, out),
                    "replace_composed": lambda: plan_n.RotateChain(level, ct_n, gens, keys_n, False, out_n),
                    "replace_host_loop": lambda: plan.RotateColumnsPow2(level, ct, k_all, pow2, acc),
                    "slot_sum": lambda: plan.RotateChain(level, ct, gens, keys, True, out),
                    "slot_sum_composed": lambda: plan_n.RotateChain(level, ct_n, gens, keys_n, True, out_n),
                    "slot_sum_host_loop": slot_sum_host_loop}

                def sync_all():
                    for s in shapes.values():
                        s[1].Sync()
                        s[0].Sync()
                # the legs agree before they are timed
                for kind in ("replace", "slot_sum"):
                    for leg in (kind, kind + "_composed", kind + "_host_loop"):
                        legs[leg]()
                    same = all(np.array_equal(out[k].get(), acc[k].get()) and np.array_equal(out[k].get(), out_n[k].get()) for k in range(2))
                    if not same:
                        raise SystemExit("the %s legs disagree at %s level %d batch %d" % (kind, name, level, batch))
                times = time_legs(legs, sync_all, args.reps, args.iters, args.warmup)
                o = {leg: summarise(v) for leg, v in times.items()}
                for kind in ("replace", "slot_sum"):
                    o[kind + "_over_host_loop"] = round(o[kind]["median"] / o[kind + "_host_loop"]["median"], 3)
                    o[kind + "_over_composed"] = round(o[kind]["median"] / o[kind + "_composed"]["median"], 3)
                    o[kind + "_composed_over_host_loop"] = round(o[kind + "_composed"]["median"] / o[kind + "_host_loop"]["median"], 3)
                o["bit_exact_between_legs"] = True
                at_level[str(batch)] = o
                print("# %s level %d batch %d: %s" % (name, level, batch, json.dumps(o)), file=sys.stderr, flush=True)
                del shapes, legs, plan, plan_n, keys, keys_n, ct, ct_n, out, out_n, acc, tmp, pow2, cQ, cP
            entry["levels"][str(level)] = at_level
        result["sets"][name] = entry
        del rings
    text = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(result, indent=1) + "\n")
    print(text)


if __name__ == "__main__":
    main()
