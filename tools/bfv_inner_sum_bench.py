#!/usr/bin/env python3
"""BFV InnerSum and the power-of-two rotation chain as one device call each (lr_bfv_inner_sum, lr_bfv_rotate_chain), timed in one process
beside the sequences they replace and beside the CPU restatement.

    python tools/bfv_inner_sum_bench.py [--sets PN14QP438,PN13QP218] [--batches 1,256] [--reps 5] [--iters 2] [--warmup 1]
                                        [--cpu-threads 16] [--cpu-cts 16]

Per parameter set and batch size, uniform ciphertexts and keys resident in HBM, one different key per step:

    inner_sum               lr_bfv_inner_sum on a default plan: log2(N) - 1 column steps and the row step, each the key switch plus one
                            fused pass
    inner_sum_no_epilogue   the same call on a plan made with lr_options::no_epilogue: each step from the separate Permute / Add launches
    parent_sequence         what the overlay did until now, through the mirror: CkksPlan.BfvPermute and two Context.Add calls per step
    rotate_chain            lr_bfv_rotate_chain, the replace chain of rotateColumnsPow2 for k = N/2 - 1 (every bit set: log2(N) - 1 steps)
    rotate_chain_host_loop  the same rotation as the BfvRotateColumnsPow2 host loop of BfvPermute calls

Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after
`warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call,
and the ratios of the medians `inner_sum_over_parent`, `no_epilogue_over_parent`, `rotate_chain_over_host_loop`, whichever way they come
out.  Before the timing the three InnerSum legs and the two rotation legs are checked to give the same bits.

`cpu_restatement`: tests/bfv_chain_ref.py's InnerSum over the C oracle, `--cpu-cts` ciphertexts on `--cpu-threads` threads (the oracle's
calls release the interpreter lock).  Prints one JSON object."""
import argparse
import concurrent.futures as cf
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

from ckks_encryptor_bench import time_legs  # noqa: E402


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN14QP438,PN13QP218")
    ap.add_argument("--batches", default="1,256")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-cts", type=int, default=16)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, sampling = pkg.ring, pkg.params, pkg.sampling
    oracle = graft.load_oracle()
    oracle.build()
    import bfv_chain_ref
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.bfv_moduli(name)[:3]
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        nQ, rows, logn = len(Q), len(Q) + len(P), N.bit_length() - 1
        beta = -(-nQ // len(P))
        keys_h = [sampling.uniform_poly(Q + P, N, 2 * beta, seed=500 + i) for i in range(logn)]      # logn - 1 column keys and the row key
        gens = bfv_chain_ref.inner_sum_elements(N)
        entry = {"N": N, "limbs_q": nQ, "limbs_p": len(P), "beta": beta, "steps_inner_sum": logn, "steps_rotate_chain": logn - 1, "batches": {}}
        for batch in [int(b) for b in args.batches.split(",")]:
            ct_h = [np.tile(sampling.uniform_poly(Q, N, 1, seed=600 + k), (batch, 1, 1)) for k in range(2)]
            plans = {}
            for shape in ("default", "no_epilogue"):
                opt = ring.Options(no_epilogue=1) if shape == "no_epilogue" else ring.Options()
                cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
                plan = ring.CkksPlan(cQ, cP, batch, options=opt)
                keys = [plan.NewSwitchingKey().set(k) for k in keys_h]
                ct = (cQ.NewPoly(batch).set(ct_h[0]), cQ.NewPoly(batch).set(ct_h[1]))
                plans[shape] = (cQ, cP, plan, keys, ct, [(cQ.NewPoly(batch), cQ.NewPoly(batch)) for _ in range(3)])
            cQ, cP, plan, keys, ct, (out, acc, tmp) = plans["default"]
            _, _, plan_n, keys_n, ct_n, (out_n, _, _) = plans["no_epilogue"]
            pow2 = {1 << i: k for i, k in enumerate(keys[:-1])}
            k_all = (N >> 1) - 1

            def parent():
                cQ.Copy(ct[0], acc[0])                                   # ctOut.Copy(ct0), bfv/evaluator.go:699
                cQ.Copy(ct[1], acc[1])
                for g, key in zip(gens, keys):
                    plan.BfvPermute(acc, g, key, tmp)                    # RotateColumns / RotateRows, :702 / :706
                    cQ.Add(tmp[0], acc[0], acc[0])                       # evaluator.Add, :703 / :707
                    cQ.Add(tmp[1], acc[1], acc[1])
            legs = {
                "inner_sum": lambda: plan.BfvInnerSum(ct, keys[:-1], keys[-1], out),
                "inner_sum_no_epilogue": lambda: plan_n.BfvInnerSum(ct_n, keys_n[:-1], keys_n[-1], out_n),
                "parent_sequence": parent,
                "rotate_chain": lambda: plan.BfvRotateColumnsPow2Chain(ct, 5, k_all, pow2, out),
                "rotate_chain_host_loop": lambda: plan.BfvRotateColumnsPow2(ct, 5, k_all, pow2, tmp)}

            def sync_all():
                for p in plans.values():
                    p[1].Sync()
                    p[0].Sync()
            # the legs agree before they are timed
            legs["rotate_chain"]()
            legs["rotate_chain_host_loop"]()
            same_rot = all(np.array_equal(out[k].get(), tmp[k].get()) for k in range(2))
            for leg in ("inner_sum", "inner_sum_no_epilogue", "parent_sequence"):
                legs[leg]()
            same_sum = all(np.array_equal(out[k].get(), acc[k].get()) and np.array_equal(out[k].get(), out_n[k].get()) for k in range(2))
            if not (same_rot and same_sum):
                raise SystemExit("the legs disagree at %s batch %d (rotation %s, inner sum %s)" % (name, batch, same_rot, same_sum))
            times = time_legs(legs, sync_all, args.reps, args.iters, args.warmup)
            o = {leg: summarise(v) for leg, v in times.items()}
            o["inner_sum_over_parent"] = round(o["inner_sum"]["median"] / o["parent_sequence"]["median"], 3)
            o["no_epilogue_over_parent"] = round(o["inner_sum_no_epilogue"]["median"] / o["parent_sequence"]["median"], 3)
            o["rotate_chain_over_host_loop"] = round(o["rotate_chain"]["median"] / o["rotate_chain_host_loop"]["median"], 3)
            o["bit_exact_between_legs"] = True
            entry["batches"][str(batch)] = o
            del plans, legs
        # the CPU restatement on threads: one oracle plan per thread
        plan_keys = [k.reshape(beta, 2, rows, N) for k in keys_h]
        ct1 = np.stack([sampling.uniform_poly(Q, N, 1, seed=600 + k)[0] for k in range(2)])

        def one(_):
            oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
            return bfv_chain_ref.inner_sum(oplan, N, Q, ct1, plan_keys[:-1], plan_keys[-1])
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(max_workers=args.cpu_threads) as ex:
            list(ex.map(one, range(args.cpu_cts)))
        cpu_s = time.perf_counter() - t0
        entry["cpu_restatement"] = {"threads": args.cpu_threads, "ciphertexts": args.cpu_cts, "seconds": round(cpu_s, 3),
                                    "inner_sums_per_s": round(args.cpu_cts / cpu_s, 3)}
        result["sets"][name] = entry
    print(json.dumps(result))


if __name__ == "__main__":
    main()
