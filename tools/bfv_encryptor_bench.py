#!/usr/bin/env python3
"""The BFV encryptor and decryptor (lr_bfv_encryptor, lr_bfv_decryptor), timed in one process.

    python tools/bfv_encryptor_bench.py [--sets PN14QP438,PN13QP218] [--batch 256] [--reps 7] [--iters 10] [--warmup 3] [--cpu 32]

Per parameter set: EncryptPk and EncryptSk, fast and through P, with the randomness resident in HBM (the device-pointer entry points: the
kernels and their launches, nothing else) and from host arrays (box to box: the copy into the pinned staging buffer and the PCIe transfer
included), and Decrypt at degrees 1 and 2.  Every repetition times each leg once, in alternating order, as `iters` back-to-back calls
between two device synchronisations (after `warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the
repetitions in microseconds per call, ciphertexts per second at the median, the bytes that cross PCIe per ciphertext (the compact
randomness; `pcie_bytes_full_polys` is what three, or one, sampled polys over Q||P would be), the algorithmic bytes per ciphertext -- the
compulsory HBM traffic: the randomness and the plaintext read, the two components written (keys are shared by the batch); for Decrypt the
components read and the plaintext written -- and the share of the 8 TB/s HBM roofline those bytes reach at the measured rate.
`cpu_restatement`: tests/bfv_encryptor_ref.py over the CPU oracle on `--cpu` ciphertexts spread over 16 threads, the baseline.
Prints one JSON object."""
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

HBM_BYTES_PER_S = 8e12


def device_bytes(ring, cQ, arrays):
    """byte arrays one behind the other in device memory (a one-limb poly as a plain buffer); returns the poly and the pointers"""
    N = cQ.N
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in arrays])
    polys = -(-flat.size // (8 * N))
    buf = np.zeros(polys * N * 8, dtype=np.uint8)
    buf[:flat.size] = flat
    poly = ring.Poly(cQ, 1, polys).set(buf.view(np.uint64).reshape(polys, 1, N))
    ptrs, off = [], 0
    for a in arrays:
        ptrs.append(poly.device_ptr + off)
        off += a.size
    return poly, ptrs


def cpu_restatement(oracle, N, Q, P, count, rng, operands):
    import bfv_encryptor_ref as ref
    enc = ref.Encryptor(oracle, N, Q, P)
    pk0, pk1, sk, crp, pt, uc, us, e0, e1 = operands
    jobs = {"pk_fast": lambda b: enc.encrypt_pk(True, pk0, pk1, uc[b], us[b], e0[b], e1[b], pt),
            "pk": lambda b: enc.encrypt_pk(False, pk0, pk1, uc[b], us[b], e0[b], e1[b], pt),
            "sk_fast": lambda b: enc.encrypt_sk(True, sk, crp, e0[b], pt),
            "sk": lambda b: enc.encrypt_sk(False, sk, crp, e0[b], pt),
            "decrypt_deg1": lambda b: ref.decrypt(enc.cQ, np.stack([pt, pt]), sk),
            "decrypt_deg2": lambda b: ref.decrypt(enc.cQ, np.stack([pt, pt, pt]), sk)}
    out = {}
    with cf.ThreadPoolExecutor(max_workers=16) as ex:
        for name, f in jobs.items():
            f(0)
            t0 = time.perf_counter()
            list(ex.map(f, [b % len(uc) for b in range(count)]))
            out[name] = round(count / (time.perf_counter() - t0), 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN14QP438,PN13QP218")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cpu", type=int, default=32, help="ciphertexts of the CPU restatement leg (0 = skip)")
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    batch = args.batch
    result = {"batch": batch, "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call",
              "hbm_bytes_per_s": HBM_BYTES_PER_S, "sets": {}}
    for name in args.sets.split(","):
        N, Q, P, _ = params.bfv_moduli(name)
        Q, P = list(Q), list(P)
        nQ, nP = len(Q), len(P)
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
        enc, dec = ring.BfvEncryptor(cQ, cP, batch), ring.BfvDecryptor(cQ, batch)
        rng = np.random.default_rng(7)
        uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
        h_pk0, h_pk1, h_sk, h_pt = uni(Q + P, 1), uni(Q + P, 1), uni(Q + P, 1), uni(Q, 1)
        qp = lambda x: ring.Poly(cQ, nQ + nP, x.shape[0]).set(x)
        pk, sk = (qp(h_pk0), qp(h_pk1)), qp(h_sk)
        h_crp = uni(Q + P, 1)
        crp = qp(np.repeat(h_crp, batch, axis=0))
        pt = cQ.NewPoly(1).set(h_pt)
        ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        ct2 = [ct[0], ct[1], cQ.NewPoly(batch)]
        out_pt = cQ.NewPoly(batch)
        uc, us = (rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8) for _ in range(2))
        e0, e1 = ((rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8) for _ in range(2))
        keep, d = device_bytes(ring, cQ, [uc, us, e0, e1])
        legs = {}
        for fast in (True, False):
            tag = "_fast" if fast else ""
            legs["pk" + tag + "_device"] = lambda fast=fast: enc.EncryptPkDevice(pk, d[0:2], d[2:4], pt, ct, fast=fast)
            legs["sk" + tag + "_device"] = lambda fast=fast: enc.EncryptSkDevice(sk, crp, d[2], pt, ct, fast=fast)
            legs["pk" + tag + "_host"] = lambda fast=fast: enc.EncryptPk(pk, (uc, us), (e0, e1), pt, ct, fast=fast)
            legs["sk" + tag + "_host"] = lambda fast=fast: enc.EncryptSk(sk, crp, e0, pt, ct, fast=fast)
        legs["decrypt_deg1"] = lambda: dec.Decrypt(ct, sk, out_pt)
        legs["decrypt_deg2"] = lambda: dec.Decrypt(ct2, sk, out_pt)
        for f in legs.values():
            for _ in range(args.warmup):
                f()
        cQ.Sync()
        times = {leg: [] for leg in legs}
        order = list(legs)
        for rep in range(args.reps):
            for leg in (order if rep % 2 == 0 else order[::-1]):
                f = legs[leg]
                cQ.Sync()
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    f()
                cQ.Sync()
                times[leg].append((time.perf_counter() - t0) / args.iters * 1e6)
        poly_q = nQ * N * 8
        out = {}
        for leg, v in times.items():
            med = statistics.median(v)
            rate = batch / med * 1e6
            row = {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1), "ciphertexts_per_s": round(rate)}
            if leg.startswith("decrypt"):
                degree = int(leg[-1])
                row["algorithmic_bytes"] = (degree + 2) * poly_q
            else:
                rand = N // 4 + 2 * N if leg.startswith("pk") else N
                row["algorithmic_bytes"] = rand + 3 * poly_q + (0 if leg.startswith("pk") else (nQ if "fast" in leg else nQ + nP) * N * 8)
                if leg.endswith("_host"):
                    row["pcie_bytes"] = rand
                    row["pcie_bytes_full_polys"] = (3 if leg.startswith("pk") else 1) * (nQ + nP) * N * 8
            row["hbm_roofline"] = round(row["algorithmic_bytes"] * rate / HBM_BYTES_PER_S, 4)
            out[leg] = row
        if args.cpu:
            oracle = graft.load_oracle()
            oracle.build()
            out["cpu_restatement_ciphertexts_per_s_16_threads"] = cpu_restatement(
                oracle, N, Q, P, args.cpu, rng, (h_pk0[0], h_pk1[0], h_sk[0], h_crp[0], h_pt[0], uc, us, e0, e1))
        result["sets"][name] = {"N": N, "limbs_q": nQ, "limbs_p": nP, "legs": out}
        del keep
    print(json.dumps(result))


if __name__ == "__main__":
    main()
