#!/usr/bin/env python3
"""Collective key switching (lr_collective), timed in one process, beside the sequence it replaces and beside the CPU restatement.

    python tools/collective_bench.py [--batch 256] [--parent-batch 32] [--fold-batch 32] [--reps 5] [--iters 2] [--warmup 1]
                                     [--cpu-threads 16] [--cpu-shares 16] [--sets ckks:PN15QP880,bfv:PN14QP438]

Per ring (CKKS PN15QP880 at the top level, BFV PN14QP438): CKS and PCKS shares for a batch of ciphertexts with one party's keys, with the
sampler bytes resident in HBM (the device-pointer entry points) and from host arrays (the copy into the pinned staging buffer and the PCIe
transfer included).  Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device
synchronisations (after `warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in
microseconds per call and shares per second at the median.

`parent_cks`, `parent_pcks`: the same shares as they had to be made before this handle existed -- the sampler bytes expanded on the host
into polys over Q||P (numpy), uploaded, lr_ntt, the lr_ewise calls of the reference's lines, lr_moddown_* -- at `--parent-batch`, timed in
the same repetitions as the handle's host-form calls at that batch.  `expand_s`, `upload_and_device_s` split their time.

`cpu_restatement`: tests/collective_ref.py over the C oracle, `--cpu-shares` shares of each protocol on `--cpu-threads` threads (the
oracle's calls release the interpreter lock).

`fold`: lr_collective_aggregate over n = 8 and n = 32 shares plus a base at `--fold-batch`, against the n lr_ewise ADD calls it replaces
(n - 1 for AggregateShares, one for KeySwitch), alternating in the same repetitions; `roofline` is the algorithmic bytes -- (n + 2) rows
of 8 N (level + 1) bytes per ciphertext -- over the median time, as a fraction of the 8 TB/s HBM spec; `not_slower` says whether the fold's
median is at most the chain's.  Prints one JSON object."""
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

HBM_BYTES_PER_S = 8e12


def summarise(v, shares):
    med = statistics.median(v)
    return {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1), "shares": shares, "shares_per_s": round(shares / med * 1e6, 1)}


def expand_noise(moduli, e):
    """KYSampler.Sample's store for [items, N] bytes: sign ? c : q - c, as [items, limbs, N] uint64"""
    c, s = (e & 127).astype(np.uint64), (e >> 7).astype(bool)
    return np.stack([np.where(s, c, np.uint64(q) - c) for q in moduli], axis=1)


def expand_ternary(oracle, moduli, uc, us, N):
    """sampleTernary at p = 0.5 for [items, N / 8] bit planes, as [items, limbs, N] uint64 in Montgomery form"""
    i = np.arange(N)
    coeff = (uc[:, i >> 3].astype(np.int64) >> (i & 7)) & 1
    sign = (us[:, i >> 3].astype(np.int64) >> (i & 7)) & 1
    index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1)
    rows = [np.array([0, oracle.mform(1, q), oracle.mform(q - 1, q)], dtype=np.uint64)[index] for q in moduli]
    return np.stack(rows, axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="ckks:PN15QP880,bfv:PN14QP438")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent-batch", type=int, default=32)
    ap.add_argument("--fold-batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-shares", type=int, default=16)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    if pkg._native.device_count() < 1:
        raise SystemExit("collective_bench needs a HIP device: nothing here is measured on the CPU")
    oracle = graft.load_oracle()
    oracle.build()
    import collective_ref
    result = {"batch": args.batch, "parent_batch": args.parent_batch, "fold_batch": args.fold_batch, "reps": args.reps, "iters": args.iters,
              "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for entry in args.sets.split(","):
        scheme, name = entry.split(":")
        if scheme == "ckks":
            N, Q, P = params.ckks_moduli(name)
        else:
            N, Q, P, _ = params.bfv_moduli(name)
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        QP, nQ, nP, rows = Q + P, len(Q), len(P), len(Q) + len(P)
        level, B, pb, fb = nQ - 1, args.batch, args.parent_batch, args.fold_batch
        cQ, cP, cQP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, QP)
        rng = np.random.default_rng(11)
        uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
        keys_h = uni(QP, 4)                                   # sk_in, sk_out, pk0, pk1: the time does not depend on the values
        sk_in, sk_out, pk0, pk1 = [ring.Poly(cQ, rows, 1).set(keys_h[i:i + 1]) for i in range(4)]
        c1_one = uni(Q, 1)
        c1 = cQ.NewPoly(B).set(np.broadcast_to(c1_one, (B, nQ, N)))
        share, o1 = cQ.NewPoly(B), cQ.NewPoly(B)
        e = [(rng.integers(0, 39, (B, N)) | (rng.integers(0, 2, (B, N)) << 7)).astype(np.uint8) for _ in range(2)]
        u = [rng.integers(0, 256, (B, N >> 3)).astype(np.uint8) for _ in range(2)]
        keep, d = device_bytes(ring, cQ, [e[0], e[1], u[0], u[1]])
        col = ring.Collective(cQ, cP, B)
        lv = (level,) if scheme == "ckks" else ()
        cks, cks_d = (col.CkksCksShare, col.CkksCksShareDevice) if scheme == "ckks" else (col.BfvCksShare, col.BfvCksShareDevice)
        pcks, pcks_d = (col.CkksPcksShare, col.CkksPcksShareDevice) if scheme == "ckks" else (col.BfvPcksShare, col.BfvPcksShareDevice)
        legs = {"cks_device": lambda: cks_d(sk_in, sk_out, c1, d[0], share, *lv),
                "cks_host": lambda: cks(sk_in, sk_out, c1, e[0], share, *lv),
                "pcks_device": lambda: pcks_d(sk_in, (pk0, pk1), c1, (d[2], d[3]), (d[0], d[1]), (share, o1), *lv),
                "pcks_host": lambda: pcks(sk_in, (pk0, pk1), c1, (u[0], u[1]), (e[0], e[1]), (share, o1), *lv)}
        times = time_legs(legs, cQ.Sync, args.reps, args.iters, args.warmup)
        out = {}
        for leg, v in times.items():
            out[leg] = summarise(v, B)
            if leg.endswith("_host"):
                out[leg]["pcie_bytes_per_share"] = N if leg.startswith("cks") else N // 4 + 2 * N
        # ---- the sequences this handle replaces, at the parent batch: host expansion, upload, lr_ntt, lr_ewise calls, lr_moddown_*
        bext = ring.FastBasisExtender(cQ, cP)
        pools = [ring.Poly(cQ, rows, pb) for _ in range(3)]
        qp = [ring.Poly.wrap(cQP, p.device_ptr, rows, pb) for p in pools]                                   # the same polys under contextQP
        qrows = [ring.Poly.wrap_strided(cQ, p.device_ptr, nQ, pb, rows) for p in pools]                     # their rows of Q ...
        prows = [ring.Poly.wrap_strided(cP, p.device_ptr + 8 * nQ * N, nP, pb, rows) for p in pools]        # ... and of P
        key_qp = [ring.Poly.wrap(cQP, k.device_ptr, rows, 1) for k in (sk_in, sk_out, pk0, pk1)]
        key_q = [ring.Poly.wrap(cQ, k.device_ptr, nQ, 1) for k in (sk_in, sk_out)]
        c1_p, out_p, out1_p, delta, tmp = cQ.NewPoly(pb).set(np.broadcast_to(c1_one, (pb, nQ, N))), cQ.NewPoly(pb), cQ.NewPoly(pb), cQ.NewPoly(1), cQ.NewPoly(pb)
        col_p = ring.Collective(cQ, cP, pb)
        cks_p, pcks_p = (col_p.CkksCksShare, col_p.CkksPcksShare) if scheme == "ckks" else (col_p.BfvCksShare, col_p.BfvPcksShare)
        ups = [ring.Poly(cQ, rows, pb) for _ in range(2)]                                                   # the expanded e0, e1 of a PCKS share
        nz = [ring.Poly.wrap(cQP, p.device_ptr, rows, pb) for p in ups]
        pscal = [int(np.prod([p % q for p in P], dtype=object)) % q for q in Q]
        split = {"parent_cks": {"expand": [], "rest": []}, "parent_pcks": {"expand": [], "rest": []}}

        def parent_cks():
            t0 = time.perf_counter()
            x = expand_noise(QP, e[0][:pb])
            t1 = time.perf_counter()
            pools[0].set(x)
            cQ.Sub(key_q[0], key_q[1], delta)
            if scheme == "ckks":
                cQP.NTT(qp[0], qp[0])
                cQ.MulCoeffsMontgomeryLvl(level, c1_p, delta, out_p)
            else:
                cQ.NTT(c1_p, tmp)
                cQ.MulCoeffsMontgomery(tmp, delta, out_p)
            cQ._ew("MUL_SCALAR_LIMBS", level, out_p, None, out_p, pscal)
            if scheme == "ckks":
                cQ.AddLvl(level, out_p, qrows[0], out_p)
                bext.ModDownSplitedNTTPQ(level, out_p, prows[0], out1_p)
            else:
                cQ.InvNTT(out_p, out_p)
                cQ.Add(out_p, qrows[0], out_p)
                bext.ModDownSplitedPQ(level, out_p, prows[0], out1_p)
            cQP.Sync()
            cP.Sync()
            cQ.Sync()
            split["parent_cks"]["expand"].append(t1 - t0)
            split["parent_cks"]["rest"].append(time.perf_counter() - t1)

        def parent_pcks():
            t0 = time.perf_counter()
            xu = expand_ternary(oracle, QP, u[0][:pb], u[1][:pb], N)
            x0, x1 = expand_noise(QP, e[0][:pb]), expand_noise(QP, e[1][:pb])
            t1 = time.perf_counter()
            pools[2].set(xu)
            cQP.NTT(qp[2], qp[2])
            ups[0].set(x0)
            ups[1].set(x1)
            for k in range(2):
                cQP.MulCoeffsMontgomery(qp[2], key_qp[2 + k], qp[k])
                if scheme == "ckks":
                    cQP.NTT(nz[k], nz[k])
                else:
                    cQP.InvNTT(qp[k], qp[k])
                cQP.Add(qp[k], nz[k], qp[k])
            for k, o in enumerate((out_p, out1_p)):
                if scheme == "ckks":
                    bext.ModDownNTTPQ(level, pools[k], o)
                else:
                    bext.ModDownPQ(level, pools[k], o)
            if scheme == "ckks":
                cQ.MulCoeffsMontgomeryAndAddLvl(level, c1_p, key_q[0], out_p)
            else:
                cQ.NTT(c1_p, tmp)
                cQ.MulCoeffsMontgomery(tmp, key_q[0], tmp)
                cQ.InvNTT(tmp, tmp)
                cQ.Add(out_p, tmp, out_p)
            cQP.Sync()
            cP.Sync()
            cQ.Sync()
            split["parent_pcks"]["expand"].append(t1 - t0)
            split["parent_pcks"]["rest"].append(time.perf_counter() - t1)

        small = {"parent_cks": parent_cks, "handle_cks_host": lambda: cks_p(sk_in, sk_out, c1_p, e[0][:pb], out_p, *lv),
                 "parent_pcks": parent_pcks,
                 "handle_pcks_host": lambda: pcks_p(sk_in, (pk0, pk1), c1_p, (u[0][:pb], u[1][:pb]), (e[0][:pb], e[1][:pb]), (out_p, out1_p), *lv)}
        ptimes = time_legs(small, cQ.Sync, max(3, args.reps // 2 + 1), 1, 1)
        cmp_ = {leg: summarise(v, pb) for leg, v in ptimes.items()}
        for leg in split:
            cmp_[leg]["expand_s"] = round(statistics.median(split[leg]["expand"]), 4)
            cmp_[leg]["upload_and_device_s"] = round(statistics.median(split[leg]["rest"]), 4)
        # ---- the CPU restatement on threads
        r = collective_ref.Collective(oracle, N, Q, P)
        jobs = {"cks": (lambda b: r.ckks_cks_share(level, keys_h[0], keys_h[1], c1_one[0], e[0][b])) if scheme == "ckks" else
                       (lambda b: r.bfv_cks_share(keys_h[0], keys_h[1], c1_one[0], e[0][b])),
                "pcks": (lambda b: r.ckks_pcks_share(level, keys_h[0], keys_h[2], keys_h[3], c1_one[0], u[0][b], u[1][b], e[0][b], e[1][b])) if scheme == "ckks" else
                        (lambda b: r.bfv_pcks_share(keys_h[0], keys_h[2], keys_h[3], c1_one[0], u[0][b], u[1][b], e[0][b], e[1][b]))}
        cpu = {}
        with cf.ThreadPoolExecutor(max_workers=args.cpu_threads) as ex:
            for what, f in jobs.items():
                f(0)
                t0 = time.perf_counter()
                list(ex.map(f, [b % B for b in range(args.cpu_shares)]))
                s = time.perf_counter() - t0
                cpu[what] = {"threads": args.cpu_threads, "shares": args.cpu_shares, "seconds": round(s, 3), "shares_per_s": round(args.cpu_shares / s, 2)}
        # ---- the fold against the chain of ADD calls, in the same repetitions
        del pools, qp, qrows, prows, ups, nz, c1, share, o1
        col_f = ring.Collective(cQ, cP, fb)
        fold = {}
        src = uni(Q, 1)
        shares = [cQ.NewPoly(fb).set(np.broadcast_to(src, (fb, nQ, N))) for _ in range(32)]
        base, out_f = cQ.NewPoly(fb).set(np.broadcast_to(src, (fb, nQ, N))), cQ.NewPoly(fb)
        for n in (8, 32):
            def chain(n=n):
                cQ.Add(shares[0], shares[1], out_f)
                for k in range(2, n):
                    cQ.Add(out_f, shares[k], out_f)
                cQ.Add(base, out_f, out_f)
            flegs = {"fold": lambda n=n: col_f.Aggregate(shares[:n], out_f, level, base=base), "add_chain": chain}
            ft = time_legs(flegs, cQ.Sync, args.reps, max(args.iters, 4), args.warmup)
            bytes_fold, bytes_chain = (n + 2) * 8 * N * nQ * fb, 3 * n * 8 * N * nQ * fb
            f_med, c_med = statistics.median(ft["fold"]), statistics.median(ft["add_chain"])
            fold["n%d" % n] = {"fold": summarise(ft["fold"], fb), "add_chain": summarise(ft["add_chain"], fb),
                               "fold_bytes": bytes_fold, "add_chain_bytes": bytes_chain,
                               "fold_roofline": round(bytes_fold / (f_med * 1e-6) / HBM_BYTES_PER_S, 3),
                               "add_chain_roofline": round(bytes_chain / (c_med * 1e-6) / HBM_BYTES_PER_S, 3),
                               "speedup": round(c_med / f_med, 2), "not_slower": bool(f_med <= c_med)}
        result["sets"][entry] = {"N": N, "limbs_q": nQ, "limbs_p": nP, "level": level, "legs": out, "against_the_parent_sequence": cmp_,
                                 "cpu_restatement": cpu, "fold": fold}
        del keep, col, col_p, col_f, shares, base, out_f
    print(json.dumps(result))


if __name__ == "__main__":
    main()
