#!/usr/bin/env python3
"""The collective Refresh (lr_refresh), timed in one process, beside the sequence it replaces and beside the CPU restatement.

    python tools/refresh_bench.py [--batch 256] [--parent-batch 2] [--reps 5] [--iters 2] [--warmup 1] [--cpu-threads 16] [--cpu-items 16]
                                  [--sets ckks:PN15QP880:0,ckks:PN15QP880:3,bfv:PN14QP438]

Per set (CKKS PN15QP880 at levelStart 0 and 3, BFV PN14QP438): GenShares for a batch of ciphertexts with one party's key, with mask and noise
resident in HBM (the device-pointer entry point) and from host arrays (the copy into the pinned staging buffer and the PCIe transfer
included), and Finalize (Decrypt, Recode, Recrypt).  Every repetition times each leg once, in alternating order, as `iters` back-to-back
calls between two device synchronisations (after `warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max)
over the repetitions in microseconds per call, and pairs of shares (or finalizes) per second at the median.

`parent_shares`, `parent_finalize`: the same results as they had to be made before this handle existed, at `--parent-batch`, timed in the
same repetitions as the handle's host-form calls at that batch.  CKKS shares: the masks reduced modulo every q_i on the host (Python
integers, as the reference's big.Int), the noise expanded on the host, both uploaded, then lr_ntt and the lr_ewise calls of the
reference's lines.  CKKS Finalize: AddLvl and InvNTTLvl on the device, the poly downloaded, PolyToBigint, the centring and
SetCoefficientsBigint in Python integers, uploaded, NTT, Add.  BFV shares: the noise expanded on the host and uploaded, lr_ntt, lr_ewise,
the two ModDowns, lift on the host.  BFV Finalize: Add, lr_simple_scale, the row downloaded, lifted on the host and uploaded, Add, the
ModDown.  `host_s`, `upload_and_device_s` split their time.

`cpu_restatement`: tests/refresh_ref.py over the C oracle, `--cpu-items` pairs of shares and finalizes on `--cpu-threads` threads (the
oracle's calls release the interpreter lock; the Python-integer lines do not).  Prints one JSON object."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import __graft_entry__ as graft  # noqa: E402

from bfv_encryptor_bench import device_bytes  # noqa: E402
from ckks_encryptor_bench import time_legs  # noqa: E402
from collective_bench import expand_noise  # noqa: E402

BFV_T = 65537


def summarise(v, items):
    med = statistics.median(v)
    return {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1), "items": items, "per_s": round(items / med * 1e6, 1)}


def plane_integers(planes):
    """word planes [W, N] of two's complement integers -> N Python integers"""
    W = planes.shape[0]
    v = sum(planes[w].astype(object) << (64 * w) for w in range(W))
    return [int(x) - (1 << (64 * W)) if int(x) >> (64 * W - 1) else int(x) for x in v]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="ckks:PN15QP880:0,ckks:PN15QP880:3,bfv:PN14QP438")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent-batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-items", type=int, default=16)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    if pkg._native.device_count() < 1:
        raise SystemExit("refresh_bench needs a HIP device: nothing here is measured on the CPU")
    oracle = graft.load_oracle()
    oracle.build()
    import refresh_ref
    result = {"batch": args.batch, "parent_batch": args.parent_batch, "reps": args.reps, "iters": args.iters, "warmup": args.warmup,
              "unit": "us per call", "sets": {}}
    for entry in args.sets.split(","):
        parts = entry.split(":")
        scheme, name = parts[0], parts[1]
        if scheme == "ckks":
            N, Q, P = params.ckks_moduli(name)
            P = []                                                        # the CKKS protocol never leaves Q
        else:
            N, Q, P, _ = params.bfv_moduli(name)
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        QP, nQ, nP, rows = Q + P, len(Q), len(P), len(Q) + len(P)
        top, B, pb = nQ - 1, args.batch, args.parent_batch
        ls = int(parts[2]) if scheme == "ckks" else top
        L1 = ls + 1
        cQ = ring.NewContextWithParams(N, Q)
        cP = ring.NewContextWithParams(N, P) if P else None
        cQP = ring.NewContextWithParams(N, QP) if P else None
        rng = np.random.default_rng(13)
        uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
        R = refresh_ref.Refresh(oracle, N, Q, P, BFV_T if scheme == "bfv" else 0)
        sk_h, c1_one, crs_one, c0_one = uni(QP, 1), uni(Q, 1), uni(QP, 1), uni(Q, 1)
        dec_one, rec_one = uni(Q, 1), uni(Q, 1)
        sk = ring.Poly(cQ, rows, 1).set(sk_h)
        wide = lambda one, limbs, n: ring.Poly(cQ, limbs, n).set(np.broadcast_to(one, (n, limbs, N)))
        c1, crs, c0 = wide(c1_one, nQ, B), wide(crs_one, rows, B), wide(c0_one, nQ, B)
        dec_in, rec_in = wide(dec_one, nQ, B), wide(rec_one, nQ, B)
        dec, rec, out0, out1 = cQ.NewPoly(B), cQ.NewPoly(B), cQ.NewPoly(B), cQ.NewPoly(B)
        e = [(rng.integers(0, 20, (B, N)) | (rng.integers(0, 2, (B, N)) << 7)).astype(np.uint8) for _ in range(2)]
        h = ring.Refresh(cQ, cP, BFV_T if scheme == "bfv" else 0, B)
        if scheme == "ckks":
            W = h.MaskWords(ls)
            mask = rng.integers(0, 1 << 63, (B, W, N), dtype=np.uint64)
            mask[:, W - 1] = np.where(rng.integers(0, 2, (B, N)) == 1, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64(0)) if W > 1 else mask[:, 0] >> np.uint64(8)
            mask_bytes = 8 * W * N
        else:
            W = 1
            mask = rng.integers(0, BFV_T, (B, N)).astype(np.uint64)
            mask_bytes = 8 * N
        keep, d = device_bytes(ring, cQ, [mask.view(np.uint8), e[0], e[1]])
        if scheme == "ckks":
            legs = {"shares_device": lambda: h.CkksGenSharesDevice(sk, ls, c1, crs, d[0], (d[1], d[2]), (dec, rec)),
                    "shares_host": lambda: h.CkksGenShares(sk, ls, c1, crs, mask, e, (dec, rec)),
                    "finalize": lambda: h.CkksFinalize(ls, c0, (dec_in, rec_in), out0)}
        else:
            legs = {"shares_device": lambda: h.BfvGenSharesDevice(sk, c1, crs, d[0], (d[1], d[2]), (dec, rec)),
                    "shares_host": lambda: h.BfvGenShares(sk, c1, crs, mask, e, (dec, rec)),
                    "finalize": lambda: h.BfvFinalize(c0, crs, (dec_in, rec_in), (out0, out1))}
        times = time_legs(legs, cQ.Sync, args.reps, args.iters, args.warmup)
        print("%s: the handle's legs timed" % entry, file=sys.stderr, flush=True)
        out = {leg: summarise(v, B) for leg, v in times.items()}
        out["shares_host"]["pcie_bytes_per_pair_of_shares"] = mask_bytes + 2 * N
        # ---- the sequences this handle replaces, at the parent batch
        hp = ring.Refresh(cQ, cP, BFV_T if scheme == "bfv" else 0, pb)
        c1_p, crs_p, c0_p = wide(c1_one, nQ, pb), wide(crs_one, rows, pb), wide(c0_one, nQ, pb)
        dec_i, rec_i = wide(dec_one, nQ, pb), wide(rec_one, nQ, pb)
        dec_p, rec_p, tmp, out_p, out1_p = [cQ.NewPoly(pb) for _ in range(5)]
        skq = ring.Poly.wrap(cQ, sk.device_ptr, nQ, 1)
        split = {"parent_shares": {"host": [], "rest": []}, "parent_finalize": {"host": [], "rest": []}}

        def sync_all():
            for c in (cQP, cP, cQ):
                if c is not None:
                    c.Sync()
        if scheme == "ckks":
            def parent_shares():
                t0 = time.perf_counter()
                m = np.stack([R.set_coefficients_bigint(plane_integers(mask[b]), nQ) for b in range(pb)])      # :66, :68 on the host
                x0, x1 = expand_noise(Q, e[0][:pb]), expand_noise(Q, e[1][:pb])
                t1 = time.perf_counter()
                dec_p.set(m)
                rec_p.set(m)
                cQ.NTTLvl(ls, dec_p, dec_p)
                cQ.NTT(rec_p, rec_p)
                cQ.MulCoeffsMontgomeryAndAddLvl(ls, c1_p, skq, dec_p)
                cQ.MulCoeffsMontgomeryAndAdd(crs_p, skq, rec_p)
                tmp.set(x0)
                cQ.NTT(tmp, tmp)
                cQ.AddLvl(ls, dec_p, tmp, dec_p)
                tmp.set(x1)
                cQ.NTT(tmp, tmp)
                cQ.Add(rec_p, tmp, rec_p)
                cQ.Neg(rec_p, rec_p)
                sync_all()
                split["parent_shares"]["host"].append(t1 - t0)
                split["parent_shares"]["rest"].append(time.perf_counter() - t1)

            def parent_finalize():
                t0 = time.perf_counter()
                cQ.AddLvl(ls, c0_p, dec_i, tmp)
                cQ.InvNTTLvl(ls, tmp, tmp)
                got = tmp.get().reshape(pb, nQ, N)
                t1 = time.perf_counter()
                Qls = refresh_ref.product(Q[:L1])
                rows_ = np.stack([R.set_coefficients_bigint([refresh_ref.centre(v, Qls) for v in R.poly_to_bigint(got[b, :L1])], nQ) for b in range(pb)])
                t2 = time.perf_counter()
                tmp.set(rows_)
                cQ.NTT(tmp, tmp)
                cQ.Add(tmp, rec_i, out_p)
                sync_all()
                split["parent_finalize"]["host"].append(t2 - t1)
                split["parent_finalize"]["rest"].append(time.perf_counter() - t2 + t1 - t0)
            small = {"parent_shares": parent_shares, "handle_shares_host": lambda: hp.CkksGenShares(skq, ls, c1_p, crs_p, mask[:pb], (e[0][:pb], e[1][:pb]), (dec_p, rec_p)),
                     "parent_finalize": parent_finalize, "handle_finalize": lambda: hp.CkksFinalize(ls, c0_p, (dec_i, rec_i), out_p)}
        else:
            bext, scaler = ring.FastBasisExtender(cQ, cP), ring.SimpleScaler(BFV_T, cQ)
            pools = [ring.Poly(cQ, rows, pb) for _ in range(3)]
            qp = [ring.Poly.wrap(cQP, p.device_ptr, rows, pb) for p in pools]                               # the same polys under contextQP
            qrows = [ring.Poly.wrap_strided(cQ, p.device_ptr, nQ, pb, rows) for p in pools]                 # their rows of Q ...
            prows = [ring.Poly.wrap_strided(cP, p.device_ptr + 8 * nQ * N, nP, pb, rows) for p in pools]    # ... and of P
            crs_qp, sk_qp = ring.Poly.wrap(cQP, crs_p.device_ptr, rows, pb), ring.Poly.wrap(cQP, sk.device_ptr, rows, 1)
            pscal = [int(np.prod([p % q for p in P], dtype=object)) % q for q in Q]

            def parent_shares():
                t0 = time.perf_counter()
                x0, x1 = expand_noise(QP, e[0][:pb]), expand_noise(QP, e[1][:pb])
                lifted = np.stack([R.lift(mask[b]) for b in range(pb)])                                     # :153 on the host
                t1 = time.perf_counter()
                pools[0].set(x0)
                pools[1].set(x1)
                cQ.NTT(c1_p, tmp)
                cQ.MulCoeffsMontgomery(tmp, skq, tmp)
                cQ.InvNTT(tmp, tmp)
                cQ._ew("MUL_SCALAR_LIMBS", top, tmp, None, tmp, pscal)
                cQ.Add(tmp, qrows[0], tmp)
                bext.ModDownSplitedPQ(top, tmp, prows[0], dec_p)
                cQP.NTT(crs_qp, qp[2])
                cQP.MulCoeffsMontgomery(qp[2], sk_qp, qp[2])
                cQP.Neg(qp[2], qp[2])
                cQP.InvNTT(qp[2], qp[2])
                cQP.Add(qp[2], qp[1], qp[2])
                bext.ModDownPQ(top, pools[2], rec_p)
                tmp.set(lifted)
                cQ.Add(dec_p, tmp, dec_p)
                cQ.Sub(rec_p, tmp, rec_p)
                sync_all()
                split["parent_shares"]["host"].append(t1 - t0)
                split["parent_shares"]["rest"].append(time.perf_counter() - t1)

            def parent_finalize():
                t0 = time.perf_counter()
                cQ.Add(c0_p, dec_i, tmp)
                scaler.Scale(tmp, tmp)
                got = tmp.get().reshape(pb, nQ, N)
                t1 = time.perf_counter()
                lifted = np.stack([R.lift(got[b, 0]) for b in range(pb)])                                   # :178 on the host
                t2 = time.perf_counter()
                tmp.set(lifted)
                cQ.Add(tmp, rec_i, out_p)
                bext.ModDownPQ(top, crs_p, out1_p)
                sync_all()
                split["parent_finalize"]["host"].append(t2 - t1)
                split["parent_finalize"]["rest"].append(time.perf_counter() - t2 + t1 - t0)
            small = {"parent_shares": parent_shares, "handle_shares_host": lambda: hp.BfvGenShares(sk, c1_p, crs_p, mask[:pb], (e[0][:pb], e[1][:pb]), (dec_p, rec_p)),
                     "parent_finalize": parent_finalize, "handle_finalize": lambda: hp.BfvFinalize(c0_p, crs_p, (dec_i, rec_i), (out_p, out1_p))}
        ptimes = time_legs(small, cQ.Sync, max(3, args.reps // 2 + 1), 1, 1)
        cmp_ = {leg: summarise(v, pb) for leg, v in ptimes.items()}
        print("%s: the parent sequence timed" % entry, file=sys.stderr, flush=True)
        for leg in split:
            cmp_[leg]["host_s"] = round(statistics.median(split[leg]["host"]), 4)
            cmp_[leg]["upload_and_device_s"] = round(statistics.median(split[leg]["rest"]), 4)
        # ---- the CPU restatement on threads
        if scheme == "ckks":
            ints = [plane_integers(mask[b]) for b in range(min(B, 4))]
            jobs = {"shares": lambda b: R.ckks_gen_shares(ls, sk_h[0], c1_one[0], crs_one[0], ints[b % len(ints)], e[0][b], e[1][b]),
                    "finalize": lambda b: R.ckks_finalize(ls, c0_one[0], dec_one[0], rec_one[0])}
        else:
            jobs = {"shares": lambda b: R.bfv_gen_shares(sk_h[0], c1_one[0], crs_one[0], mask[b], e[0][b], e[1][b]),
                    "finalize": lambda b: R.bfv_finalize(c0_one[0], crs_one[0], dec_one[0], rec_one[0])}
        cpu = {}
        with cf.ThreadPoolExecutor(max_workers=args.cpu_threads) as ex:
            for what, f in jobs.items():
                f(0)
                t0 = time.perf_counter()
                list(ex.map(f, [b % B for b in range(args.cpu_items)]))
                s = time.perf_counter() - t0
                cpu[what] = {"threads": args.cpu_threads, "items": args.cpu_items, "seconds": round(s, 3), "per_s": round(args.cpu_items / s, 2)}
        result["sets"][entry] = {"N": N, "limbs_q": nQ, "limbs_p": nP, "level_start": ls, "mask_words": W, "legs": out,
                                 "against_the_parent_sequence": cmp_, "cpu_restatement": cpu}
        print("%s: the CPU restatement timed" % entry, file=sys.stderr, flush=True)
        del keep, h, hp
    print(json.dumps(result))


if __name__ == "__main__":
    main()
