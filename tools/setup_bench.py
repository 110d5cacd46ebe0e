#!/usr/bin/env python3
"""The collective key setup (lr_setup), timed in one process, beside the sequence it replaces and beside the CPU restatement.

    python tools/setup_bench.py [--sets ckks:PN15QP880,bfv:PN14QP438] [--reps 5] [--iters 2] [--warmup 1] [--cpu-threads 16] [--cpu-parties 4]

Per parameter set, per party (one party per call, its keys shared by nothing), with the sampler bytes resident in HBM (the device-pointer
entry points) and, for round one, from host arrays (the copy into the pinned staging buffer and the PCIe transfer included):

    ckg_share                 one CKG share
    rkg_three_rounds          rounds one, two and three of RKG back to back (the aggregates they read are resident)
    rkg_naive                 rounds one and two of the naive RKG
    rtg_pow2                  the power-of-two rotation set: 2 (logN - 1) + 1 RTG shares in ONE call
    rkg_key, rtg_key          the finalize steps
    fold_3, fold_32           lr_setup_aggregate over 3 and 32 shares of beta pairs

each under a handle of the default (fused) shape and under one made with lr_options::no_epilogue (one launch per Context call), in the
same repetitions: `fused_over_call_by_call` is the ratio of the medians, reported whichever way it comes out.  Every repetition times
each leg once, in alternating order, as `iters` back-to-back calls between two device synchronisations (after `warmup` untimed calls per
leg).  Reported per leg: the median and the spread (min, max) over the repetitions in microseconds per call.

`parent_sequence`: round one of RKG for one party as it had to be made on the device before this handle existed -- the Gaussian bytes
expanded on the host into beta polys over Q||P (numpy), uploaded, lr_ntt, MUL_SCALAR_LIMBS and INV_MFORM on a copy of sk, then per digit
the lr_ewise calls ADD on the digit's rows and MUL_MONT_AND_SUB -- timed in the same repetitions as `rkg_round1_host`, the new entry
point.  `expand_s`, `upload_and_device_s` split its time.

`cpu_restatement`: tests/setup_ref.py over the C oracle, round one of `--cpu-parties` parties on `--cpu-threads` threads (the oracle's
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

from bfv_encryptor_bench import device_bytes  # noqa: E402
from ckks_encryptor_bench import time_legs  # noqa: E402
from keygen_bench import expand_on_host  # noqa: E402


def summarise(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="ckks:PN15QP880,bfv:PN14QP438")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-parties", type=int, default=4)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    oracle = graft.load_oracle()
    oracle.build()
    import setup_ref
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for entry in args.sets.split(","):
        scheme, name = entry.split(":")
        N, Q, P = (params.ckks_moduli(name) if scheme == "ckks" else params.bfv_moduli(name))[:3]
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        QP, nQ, rows = Q + P, len(Q), len(Q) + len(P)
        beta = -(-nQ // len(P))
        rng = np.random.default_rng(7)
        uni = lambda n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in QP], dtype=np.uint64) for _ in range(n)])
        n_rot = 2 * (N.bit_length() - 2) + 1
        noise = lambda *shape: (rng.integers(0, 20, shape + (N,)) | (rng.integers(0, 2, shape + (N,)) << 7)).astype(np.uint8)
        e1, e2, e_rot = noise(1, beta), noise(1, beta, 2), noise(n_rot, beta)
        bits = rng.integers(0, 256, (2, 1, beta, N >> 3)).astype(np.uint8)
        sk_h, u_h, crs_h, crp_h, pairs_h = uni(1), uni(1), uni(1), uni(beta), uni(2 * beta)
        legs, handles = {}, []
        for shape in ("fused", "call_by_call"):
            opt = ring.Options(no_epilogue=1) if shape == "call_by_call" else ring.Options()
            cQ, cP = ring.NewContextWithParams(N, Q, options=opt), ring.NewContextWithParams(N, P, options=opt)
            st = ring.Setup(cQ, cP, n_rot, options=opt)
            gens = ring.KeyGenerator(cQ, cP, 1).Pow2GaloisElements()
            keep, d = device_bytes(ring, cQ, [e1, e2, e_rot, bits[0], bits[1]])
            sk, u, crs = (st.NewPoly().set(x) for x in (sk_h, u_h, crs_h))
            crp, r1, r3 = (st.NewShare().set(crp_h) for _ in range(3))
            r2, evk = st.NewPairShare().set(pairs_h), st.NewPairShare()
            ckg, s1, s2 = st.NewPoly(), [st.NewShare()], [st.NewPairShare()]
            rot = [st.NewShare() for _ in range(n_rot)]
            terms = [st.NewPairShare().set(pairs_h) for _ in range(32)]
            handles.append((cQ, cP, st, keep, sk, u, crs, crp, r1, r2, r3, evk, ckg, s1, s2, rot, terms))
            scheme_id = st.CKKS if scheme == "ckks" else st.BFV

            def three(st=st, u=u, sk=sk, crp=crp, r1=r1, r2=r2, s1=s1, s2=s2, d=d):
                st.RkgRound1Device(u, sk, crp, d[0], s1)
                st.RkgRound2Device(r1, sk, crp, d[1], s2)
                st.RkgRound3Device(r2, u, sk, d[0], s1)

            def naive(st=st, sk=sk, crs=crs, r2=r2, s2=s2, d=d, scheme_id=scheme_id):
                st.RkgNaiveRound1Device(scheme_id, sk, (crs, crs), d[1], (d[3], d[4]), s2)
                st.RkgNaiveRound2Device(r2, sk, (crs, crs), (d[3], d[4]), d[1], s2)
            legs.update({
                shape + ".ckg_share": lambda st=st, sk=sk, crs=crs, d=d, ckg=ckg: st.CkgShareDevice(sk, crs, d[0], ckg),
                shape + ".rkg_three_rounds": three,
                shape + ".rkg_naive": naive,
                shape + ".rtg_pow2": lambda st=st, sk=sk, gens=gens, crp=crp, d=d, rot=rot: st.RtgShareDevice(sk, gens, crp, d[2], rot),
                shape + ".rkg_key": lambda st=st, r2=r2, r3=r3, evk=evk: st.RkgKey(r2, r3, evk),
                shape + ".rtg_key": lambda st=st, r1=r1, crp=crp, evk=evk: st.RtgKey(r1, crp, evk),
                shape + ".fold_3": lambda st=st, terms=terms, evk=evk: st.Aggregate(terms[:3], evk),
                shape + ".fold_32": lambda st=st, terms=terms, evk=evk: st.Aggregate(terms, evk)})

        def sync_all():
            for h in handles:
                h[1].Sync()
                h[0].Sync()
        times = time_legs(legs, sync_all, args.reps, args.iters, args.warmup)
        out = {"fused": {}, "call_by_call": {}, "fused_over_call_by_call": {}}
        for leg, v in times.items():
            shape, what = leg.split(".")
            out[shape][what] = summarise(v)
        for what in out["fused"]:
            out["fused_over_call_by_call"][what] = round(out["fused"][what]["median"] / out["call_by_call"][what]["median"], 3)
        out["rtg_shares_per_call"] = n_rot
        # the sequence this handle replaces, round one of RKG for one party: host expansion, upload, lr_ntt, lr_ewise calls per digit
        cQ, cP, st, _, sk, u, crs, crp = handles[0][:8]
        s1 = handles[0][13]
        cQP = ring.NewContextWithParams(N, QP)
        share, tmp = ring.Poly(cQ, rows, beta), ring.Poly(cQ, rows, 1)
        pscal = [int(np.prod([p % q for p in P], dtype=object)) % q for q in Q]
        stride = rows * N * 8

        def member(poly, i, limb0, limbs, ctx):
            return ring.Poly.wrap(ctx, poly.device_ptr + i * stride + limb0 * N * 8, limbs, 1)
        digits = [(i * len(P), min((i + 1) * len(P), nQ)) for i in range(beta)]
        rings_digit = [ring.NewContextWithParams(N, Q[d0:d1]) for d0, d1 in digits]
        view = ring.Poly.wrap(cQP, share.device_ptr, rows, beta)
        sk_q, tmp_q, u_qp = member(sk, 0, 0, nQ, cQ), member(tmp, 0, 0, nQ, cQ), member(u, 0, 0, rows, cQP)
        sh = [member(share, i, 0, rows, cQP) for i in range(beta)]
        cr = [member(crp, i, 0, rows, cQP) for i in range(beta)]
        sh_d = [member(share, i, d0, d1 - d0, c) for i, ((d0, d1), c) in enumerate(zip(digits, rings_digit))]
        tmp_d = [member(tmp, 0, d0, d1 - d0, c) for (d0, d1), c in zip(digits, rings_digit)]
        split = {"expand": [], "rest": []}

        def parent():
            t0 = time.perf_counter()
            x = expand_on_host(QP, e1[0], N)
            t1 = time.perf_counter()
            share.set(x)
            cQP.NTT(view, view)
            cQ._ew("MUL_SCALAR_LIMBS", nQ - 1, sk_q, None, tmp_q, pscal)
            cQ._ew("INV_MFORM", nQ - 1, tmp_q, None, tmp_q)
            for i in range(beta):
                rings_digit[i].Add(sh_d[i], tmp_d[i], sh_d[i])
                cQP.MulCoeffsMontgomeryAndSub(u_qp, cr[i], sh[i])
            for c in rings_digit:
                c.Sync()
            cQP.Sync()
            cQ.Sync()
            split["expand"].append(t1 - t0)
            split["rest"].append(time.perf_counter() - t1)
        small = {"parent_sequence": parent, "rkg_round1_host": lambda: st.RkgRound1(u, sk, crp, e1, s1)}
        ptimes = time_legs(small, sync_all, max(3, args.reps // 2 + 1), 1, 1)
        cmp_ = {leg: summarise(v) for leg, v in ptimes.items()}
        cmp_["parent_sequence"]["expand_s"] = round(statistics.median(split["expand"]), 4)
        cmp_["parent_sequence"]["upload_and_device_s"] = round(statistics.median(split["rest"]), 4)
        cmp_["rkg_round1_host"]["pcie_bytes"] = beta * N
        cmp_["rkg_round1_host"]["pcie_bytes_uploaded_whole"] = beta * rows * N * 8
        # the CPU restatement on threads
        r = setup_ref.Setup(oracle, N, Q, P, scheme)
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(max_workers=args.cpu_threads) as ex:
            list(ex.map(lambda k: r.rkg_round1(u_h[0], sk_h[0], crp_h, e1[0]), range(args.cpu_parties)))
        cpu_s = time.perf_counter() - t0
        cmp_["cpu_restatement"] = {"threads": args.cpu_threads, "parties": args.cpu_parties, "seconds": round(cpu_s, 3),
                                   "round1_shares_per_s": round(args.cpu_parties / cpu_s, 3)}
        result["sets"][entry] = {"N": N, "limbs_q": nQ, "limbs_p": len(P), "beta": beta, "legs": out, "rkg_round_one": cmp_}
        del handles, legs
    print(json.dumps(result))


if __name__ == "__main__":
    main()
