#!/usr/bin/env python3
"""The CKKS encryptor (lr_ckks_encryptor), timed in one process, beside the only way to do the same job without it.

    python tools/ckks_encryptor_bench.py [--sets PN15QP880,PN16QP1761] [--batch 256] [--parent-batch 32] [--reps 5] [--iters 3] [--warmup 2]

Per parameter set, at the top level: EncryptPk and EncryptSk, fast and through P, with the randomness resident in HBM (the device-pointer
entry points: the kernels and their launches, nothing else) and from host arrays (box to box: the copy into the pinned staging buffer and
the PCIe transfer included).  Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two device
synchronisations (after `warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the repetitions in
microseconds per call, ciphertexts per second at the median and the bytes that cross PCIe per ciphertext.  `--batch` is halved until
the handle and its operands fit in device memory; the batch in use is reported.

`parent_sequence`: pk through P as it had to be done before this entry point existed -- the same compact decisions expanded on the host
into u, e0 and e1 over Q||P (numpy, vectorised over the batch), uploaded, lr_ntt of u, then lr_ckks_encrypt_pk -- at `--parent-batch`
ciphertexts per call (three full polys per ciphertext on the host: 60 MB at PN16QP1761), with `pk_host` of the new entry point timed at the
same batch in the same repetitions.  `expand_s`, `upload_and_encrypt_s` split the parent's time.  Prints one JSON object."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import __graft_entry__ as graft  # noqa: E402

from bfv_encryptor_bench import device_bytes  # noqa: E402


def expand_on_host(moduli, uc, us, e0, e1, N):
    """the samplers' stores for a batch: u = matrixTernaryMontgomery[limb][index], e_k = sign ? c : q - c, as [batch, limbs, N] uint64"""
    i = np.arange(N)
    coeff = (uc[:, i >> 3] >> (i & 7).astype(np.uint8)) & 1
    sign = (us[:, i >> 3] >> (i & 7).astype(np.uint8)) & 1
    index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1)
    u = np.stack([np.array([0, (1 << 64) % q, ((q - 1) << 64) % q], dtype=np.uint64)[index] for q in moduli], axis=1)
    out = [u]
    for e in (e0, e1):
        c, s = (e & 127).astype(np.uint64), (e >> 7).astype(bool)
        out.append(np.stack([np.where(s, c, np.uint64(q) - c) for q in moduli], axis=1))
    return out


def time_legs(legs, sync, reps, iters, warmup):
    for f in legs.values():
        for _ in range(warmup):
            f()
    sync()
    times = {leg: [] for leg in legs}
    order = list(legs)
    for rep in range(reps):
        for leg in (order if rep % 2 == 0 else order[::-1]):
            sync()
            t0 = time.perf_counter()
            for _ in range(iters):
                legs[leg]()
            sync()
            times[leg].append((time.perf_counter() - t0) / iters * 1e6)
    return times


def summarise(v, batch):
    med = statistics.median(v)
    return {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1), "ciphertexts_per_s": round(batch / med * 1e6, 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--parent-batch", type=int, default=32)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params, nat = pkg.ring, pkg.params, pkg._native
    result = {"batch_asked": args.batch, "reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.ckks_moduli(name)
        Q, P = list(Q), list(P)
        nQ, nP, level = len(Q), len(P), len(Q) - 1
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
        rng = np.random.default_rng(7)
        uni = lambda moduli, n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(n)])
        qp = lambda x: ring.Poly(cQ, nQ + nP, x.shape[0]).set(x)
        pk, sk, pt = (qp(uni(Q + P, 1)), qp(uni(Q + P, 1))), qp(uni(Q + P, 1)), cQ.NewPoly(1).set(uni(Q, 1))
        batch = args.batch
        while True:         # the largest batch that fits: the handle's pool is 3 polys over Q||P per ciphertext, crp one, the ciphertext two over Q
            try:
                enc = ring.CkksEncryptor(cQ, cP, batch)
                crp, ct = ring.Poly(cQ, nQ + nP, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
                break
            except nat.LatticeRingError:
                enc = crp = ct = None
                if batch == 1:
                    raise
                batch //= 2
        chunk = uni(Q + P, 1)
        for b in range(batch):          # the same uniform poly in every slot: the time does not depend on the values
            ring.Poly.wrap(cQ, crp.device_ptr + b * (nQ + nP) * N * 8, nQ + nP, 1).set(chunk)
        uc, us = (rng.integers(0, 256, (batch, N >> 3)).astype(np.uint8) for _ in range(2))
        e0, e1 = ((rng.integers(0, 20, (batch, N)) | (rng.integers(0, 2, (batch, N)) << 7)).astype(np.uint8) for _ in range(2))
        keep, d = device_bytes(ring, cQ, [uc, us, e0, e1])
        legs = {}
        for fast in (True, False):
            tag = "_fast" if fast else ""
            legs["pk" + tag + "_device"] = lambda fast=fast: enc.EncryptPkDevice(pk, d[0:2], d[2:4], pt, ct, level, fast=fast)
            legs["sk" + tag + "_device"] = lambda fast=fast: enc.EncryptSkDevice(sk, crp, d[2], pt, ct, level, fast=fast)
            legs["pk" + tag + "_host"] = lambda fast=fast: enc.EncryptPk(pk, (uc, us), (e0, e1), pt, ct, level, fast=fast)
            legs["sk" + tag + "_host"] = lambda fast=fast: enc.EncryptSk(sk, crp, e0, pt, ct, level, fast=fast)
        times = time_legs(legs, cQ.Sync, args.reps, args.iters, args.warmup)
        out = {}
        for leg, v in times.items():
            row = summarise(v, batch)
            if leg.endswith("_host"):
                row["pcie_bytes"] = N // 4 + 2 * N if leg.startswith("pk") else N
                row["pcie_bytes_full_polys"] = (3 if leg.startswith("pk") else 1) * (nQ + nP) * N * 8
            out[leg] = row
        # the parent sequence beside the new entry point, same decisions, same batch, same repetitions
        pb = min(args.parent_batch, batch)
        plan = ring.CkksPlan(cQ, cP, pb)
        full = [ring.Poly(cQ, nQ + nP, pb) for _ in range(3)]
        pct = (cQ.NewPoly(pb), cQ.NewPoly(pb))
        cQP = ring.NewContextWithParams(N, Q + P)
        split = {"expand": [], "rest": []}

        def parent():
            t0 = time.perf_counter()
            u, x0, x1 = expand_on_host(Q + P, uc[:pb], us[:pb], e0[:pb], e1[:pb], N)
            t1 = time.perf_counter()
            for poly, a in zip(full, (u, x0, x1)):
                poly.set(a)
            view = ring.Poly.wrap(cQP, full[0].device_ptr, nQ + nP, pb)
            cQP.NTT(view, view)
            plan.EncryptPk(level, full[0], pk, (full[1], full[2]), pt, pct)
            cQ.Sync()
            split["expand"].append(t1 - t0)
            split["rest"].append(time.perf_counter() - t1)

        small = {"parent_sequence": parent,
                 "pk_host": lambda: enc.EncryptPk(pk, (uc[:pb], us[:pb]), (e0[:pb], e1[:pb]), pt, pct, level, fast=False)}
        ptimes = time_legs(small, cQ.Sync, max(3, args.reps // 2 + 1), 1, 1)
        cmp_ = {leg: summarise(v, pb) for leg, v in ptimes.items()}
        cmp_["parent_sequence"]["expand_s"] = round(statistics.median(split["expand"]), 4)
        cmp_["parent_sequence"]["upload_and_encrypt_s"] = round(statistics.median(split["rest"]), 4)
        cmp_["batch"] = pb
        cmp_["new_over_parent"] = round(cmp_["pk_host"]["ciphertexts_per_s"] / cmp_["parent_sequence"]["ciphertexts_per_s"], 2)
        result["sets"][name] = {"N": N, "limbs_q": nQ, "limbs_p": nP, "level": level, "batch": batch, "legs": out, "pk_through_p_against_parent": cmp_}
        del keep, enc, crp, ct, plan, full, pct
    print(json.dumps(result))


if __name__ == "__main__":
    main()
