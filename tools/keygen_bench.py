#!/usr/bin/env python3
"""The key generator (lr_keygen), timed in one process, beside the sequence it replaces and beside the CPU restatement.

    python tools/keygen_bench.py [--sets PN15QP880,PN16QP1761] [--reps 5] [--iters 2] [--warmup 1] [--cpu-threads 16] [--cpu-keys 4]

Per parameter set: one relinearisation key (GenRelinKey) and the full power-of-two rotation set (GenRotationKeysPow2: 2 (logN - 1) + 1
keys in one call), with the sampler bytes resident in HBM (the device-pointer entry points) and from host arrays (the copy into the pinned
staging buffer and the PCIe transfer included).  The uniform halves are in the key images before the clock starts, as they are for a
caller that keeps them there.  Every repetition times each leg once, in alternating order, as `iters` back-to-back calls between two
device synchronisations (after `warmup` untimed calls per leg).  Reported per leg: the median and the spread (min, max) over the
repetitions in microseconds per call and keys per second at the median.

`parent_sequence`: one rotation key as it had to be made on the device before this handle existed -- the Gaussian bytes expanded on the
host into beta polys over Q||P (numpy), uploaded together with the uniform halves, lr_ntt, then per key lr_permute_ntt and
MUL_SCALAR_LIMBS and per digit the lr_ewise calls MFORM, ADD on the digit's rows, MUL_MONT_AND_SUB -- timed in the same repetitions as
`rotation_one_host`, the new entry point for one key.  `expand_s`, `upload_and_device_s` split its time.

`cpu_restatement`: tests/keygen_ref.py over the C oracle, `--cpu-keys` rotation keys on `--cpu-threads` threads (the oracle's calls
release the interpreter lock).  Prints one JSON object."""
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


def summarise(v, keys):
    med = statistics.median(v)
    return {"median": round(med, 1), "min": round(min(v), 1), "max": round(max(v), 1), "keys": keys, "keys_per_s": round(keys / med * 1e6, 2)}


def expand_on_host(moduli, e, N):
    """KYSampler.Sample's store for [items, N] bytes: sign ? c : q - c, as [items, limbs, N] uint64"""
    c, s = (e & 127).astype(np.uint64), (e >> 7).astype(bool)
    return np.stack([np.where(s, c, np.uint64(q) - c) for q in moduli], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="PN15QP880,PN16QP1761")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-threads", type=int, default=16)
    ap.add_argument("--cpu-keys", type=int, default=4)
    args = ap.parse_args()
    pkg = graft.load_package()
    ring, params = pkg.ring, pkg.params
    oracle = graft.load_oracle()
    oracle.build()
    import keygen_ref
    result = {"reps": args.reps, "iters": args.iters, "warmup": args.warmup, "unit": "us per call", "sets": {}}
    for name in args.sets.split(","):
        N, Q, P = params.ckks_moduli(name)
        Q, P = [int(q) for q in Q], [int(p) for p in P]
        QP, nQ, rows = Q + P, len(Q), len(Q) + len(P)
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
        rng = np.random.default_rng(7)
        uni = lambda n: np.stack([np.array([rng.integers(0, q, N, dtype=np.uint64) for q in QP], dtype=np.uint64) for _ in range(n)])
        kg = ring.KeyGenerator(cQ, cP, 2 * (N.bit_length() - 2) + 1)
        beta, gens = kg.beta, kg.Pow2GaloisElements()
        n_rot = len(gens)
        sk_h, a_h = uni(1), uni(2 * beta)
        sk = ring.Poly(cQ, rows, 1).set(sk_h)
        keys = [kg.NewSwitchingKey().set(a_h) for _ in range(n_rot)]          # the same uniform polys in every key: the time does not depend on the values
        e = (rng.integers(0, 20, (n_rot, beta, N)) | (rng.integers(0, 2, (n_rot, beta, N)) << 7)).astype(np.uint8)
        keep, d = device_bytes(ring, cQ, [e])
        legs = {"relin_device": lambda: kg.GenRelinKeysDevice(sk, d[0], keys[:1]),
                "relin_host": lambda: kg.GenRelinKeys(sk, e[:1], keys[:1]),
                "rotation_pow2_device": lambda: kg.GenRotationKeysDevice(sk, gens, d[0], keys),
                "rotation_pow2_host": lambda: kg.GenRotationKeys(sk, gens, e, keys)}
        times = time_legs(legs, cQ.Sync, args.reps, args.iters, args.warmup)
        out = {}
        for leg, v in times.items():
            n = 1 if leg.startswith("relin") else n_rot
            out[leg] = summarise(v, n)
            if leg.endswith("_host"):
                out[leg]["pcie_bytes_per_key"] = beta * N
                out[leg]["pcie_bytes_per_key_uploaded_whole"] = 2 * beta * rows * N * 8
        # the sequence this handle replaces, one rotation key: host expansion, upload of both halves, lr_ntt, lr_ewise calls
        cQP = ring.NewContextWithParams(N, QP)
        noise, key, skin = ring.Poly(cQ, rows, beta), kg.NewSwitchingKey(), ring.Poly(cQ, rows, 1)
        pscal = [int(np.prod([p % q for p in P], dtype=object)) % q for q in Q]
        split = {"expand": [], "rest": []}
        stride = rows * N * 8

        def member(poly, i, limb0, limbs, ctx):
            return ring.Poly.wrap(ctx, poly.device_ptr + i * stride + limb0 * N * 8, limbs, 1)

        # everything a caller of the old sequence keeps between calls is made before the clock starts: the views of the polys, one
        # context per digit over the digit's own moduli (ONE Add on the digit's rows), the host image with the uniform halves
        digits = [(i * len(P), min((i + 1) * len(P), nQ)) for i in range(beta)]
        rings_digit = [ring.NewContextWithParams(N, Q[d0:d1]) for d0, d1 in digits]
        view = ring.Poly.wrap(cQP, noise.device_ptr, rows, beta)
        sk_q, skin_q, sk_qp = member(sk, 0, 0, nQ, cQ), member(skin, 0, 0, nQ, cQ), member(sk, 0, 0, rows, cQP)
        ev = [member(key, 2 * i, 0, rows, cQP) for i in range(beta)]
        od = [member(key, 2 * i + 1, 0, rows, cQP) for i in range(beta)]
        en = [member(noise, i, 0, rows, cQP) for i in range(beta)]
        ev_d = [member(key, 2 * i, d0, d1 - d0, c) for i, ((d0, d1), c) in enumerate(zip(digits, rings_digit))]
        skin_d = [member(skin, 0, d0, d1 - d0, c) for (d0, d1), c in zip(digits, rings_digit)]
        img = np.zeros((2 * beta, rows, N), dtype=np.uint64)
        img[1::2] = a_h[1::2]

        def parent():
            t0 = time.perf_counter()
            x = expand_on_host(QP, e[0], N)
            t1 = time.perf_counter()
            noise.set(x)
            key.set(img)                                                   # both halves cross: the even ones as zeros
            cQP.NTT(view, view)
            cQ.PermuteNTTLvl(nQ - 1, sk_q, gens[0], skin_q)
            cQ._ew("MUL_SCALAR_LIMBS", nQ - 1, skin_q, None, skin_q, pscal)
            for i in range(beta):
                cQP.MForm(en[i], ev[i])
                rings_digit[i].Add(ev_d[i], skin_d[i], ev_d[i])
                cQP.MulCoeffsMontgomeryAndSub(od[i], sk_qp, ev[i])
            for c in rings_digit:
                c.Sync()
            cQP.Sync()
            cQ.Sync()
            split["expand"].append(t1 - t0)
            split["rest"].append(time.perf_counter() - t1)

        small = {"parent_sequence": parent, "rotation_one_host": lambda: kg.GenRotationKeys(sk, gens[:1], e[:1], keys[:1])}
        ptimes = time_legs(small, cQ.Sync, max(3, args.reps // 2 + 1), 1, 1)
        cmp_ = {leg: summarise(v, 1) for leg, v in ptimes.items()}
        cmp_["parent_sequence"]["expand_s"] = round(statistics.median(split["expand"]), 4)
        cmp_["parent_sequence"]["upload_and_device_s"] = round(statistics.median(split["rest"]), 4)
        # the CPU restatement on threads
        r = keygen_ref.KeyGenerator(oracle, N, Q, P, "ckks")
        a_ref = a_h[1::2]
        t0 = time.perf_counter()
        with cf.ThreadPoolExecutor(max_workers=args.cpu_threads) as ex:
            list(ex.map(lambda k: r.gen_rot_key(sk_h[0], gens[k % n_rot], e[k % n_rot], a_ref), range(args.cpu_keys)))
        cpu_s = time.perf_counter() - t0
        cmp_["cpu_restatement"] = {"threads": args.cpu_threads, "keys": args.cpu_keys, "seconds": round(cpu_s, 3), "keys_per_s": round(args.cpu_keys / cpu_s, 3)}
        result["sets"][name] = {"N": N, "limbs_q": nQ, "limbs_p": len(P), "beta": beta, "rotation_keys": n_rot, "legs": out, "one_rotation_key": cmp_}
        del keep, kg, keys, noise, key, skin
    print(json.dumps(result))


if __name__ == "__main__":
    main()
