"""Test helper (not a test module): the CKKS rotation chains -- rotateColumnsPow2 (ckks/evaluator.go:1402-1424) and the slot-sum loop
RotateColumns(ct, 2^i, tmp); Add(ct, tmp, ct) -- composed from the CPU oracle as it stands: oplan.permute_ntt (evaluator.permuteNTT,
:1452-1471) per step and evaluator.Add at equal scales as (r + a) mod q_i in numpy per limb (both operands are below q_i < 2^62, so the
sum fits a uint64 and CRed(r + a) is the remainder).  One ciphertext at a time: ct is [2, level + 1, N] uint64 in the NTT domain, a key is
[beta, 2, |Q| + |P|, N] as the oracle's key switch reads it."""
import numpy as np

GALOIS_GEN = 5      # ckks/ckks.go


def pow2_steps(N, k, left=True):
    """rotateColumnsPow2's loop (:1414-1423): [(Galois element, key index 2^i)] for the set bits of k; the element of the rotation by 2^i
    is 5^(2^i) mod 2N to the left and 5^(-2^i) mod 2N to the right (ckks/keygen.go: ring.PermuteNTTIndex(GaloisGen, +-2^i, N))"""
    out, idx = [], 1
    g = GALOIS_GEN if left else pow(GALOIS_GEN, -1, 2 * N)
    while k > 0:
        if k & 1:
            out.append((pow(g, idx, 2 * N), idx))
        idx <<= 1
        k >>= 1
    return out


def slot_sum_elements(N):
    """5^(2^i) mod 2N for 2^i < N / 2: after the accumulating chain over them every slot holds the sum of the N / 2 slots"""
    out, i = [], 1
    while i < N >> 1:
        out.append(pow(GALOIS_GEN, i, 2 * N))
        i <<= 1
    return out


def chain(oplan, level, Q, ct, gens, keys, accumulate):
    """the state after the steps (gens[i], keys[i]): replaced by the rotation (rotateColumnsPow2 :1423) or added to it (Add)"""
    q = np.array([int(x) for x in Q[:level + 1]], dtype=np.uint64)[None, :, None]
    a = np.array(ct, dtype=np.uint64)
    for g, key in zip(gens, keys):
        r = oplan.permute_ntt(level, a, int(g), key)
        a = (r + a) % q if accumulate else r
    return a


def rotate_columns_pow2(oplan, level, N, Q, ct, k, pow2_keys, left=True):
    """rotateColumnsPow2(ct, k, evakeyRotCol): pow2_keys = {2^i: key}"""
    steps = pow2_steps(N, k, left)
    return chain(oplan, level, Q, ct, [g for g, _ in steps], [pow2_keys[i] for _, i in steps], False)
