"""Test helper (not a test module): bfv.evaluator.InnerSum (bfv/evaluator.go:691-708) and rotateColumnsPow2 (:637-666) composed from the
CPU oracle as it stands -- oplan.bfv_permute (evaluator.permute, :711-733) per step and evaluator.Add as (x + y) mod q_i in numpy per limb
(both operands are below q_i < 2^62, so the sum fits a uint64 and CRed(x + y) is the remainder).  One ciphertext at a time: ct is
[2, |Q|, N] uint64 in the coefficient domain, a key is [beta, 2, |Q| + |P|, N] as the oracle's key switch reads it."""
import numpy as np

GALOIS_GEN = 5      # bfv/bfv.go


def inner_sum_elements(N):
    """galElRotColLeft[2^i] = 5^(2^i) mod 2N for 2^i < N / 2 (InnerSum's loop, :701-702), then galElRotRow = 2N - 1 (:706)"""
    out, i = [], 1
    while i < N >> 1:
        out.append(pow(GALOIS_GEN, i, 2 * N))
        i <<= 1
    return out + [2 * N - 1]


def pow2_steps(N, generator, k):
    """rotateColumnsPow2's loop (:653-665): [(Galois element, key index 2^i)] for the set bits of k, the generator squared at every bit"""
    out, idx, mask = [], 1, 2 * N - 1
    while k > 0:
        if k & 1:
            out.append((generator, idx))
        generator = generator * generator & mask
        idx <<= 1
        k >>= 1
    return out


def chain(oplan, Q, ct, gens, keys, accumulate):
    """the state after the steps (gens[i], keys[i]): replaced by the rotation (rotateColumnsPow2 :657) or added to it (InnerSum :703, :707)"""
    q = np.array([int(x) for x in Q], dtype=np.uint64)[None, :, None]
    a = np.array(ct, dtype=np.uint64)
    for g, key in zip(gens, keys):
        r = oplan.bfv_permute(a, int(g), key)
        a = (r + a) % q if accumulate else r
    return a


def inner_sum(oplan, N, Q, ct, col_keys, row_key):
    """InnerSum: col_keys[i] = evakeyRotColLeft[2^i], i = 0 .. log2(N) - 2; row_key = evakeyRotRow"""
    gens = inner_sum_elements(N)
    assert len(col_keys) == len(gens) - 1
    return chain(oplan, Q, ct, gens, list(col_keys) + [row_key], True)


def rotate_columns_pow2(oplan, N, Q, ct, generator, k, pow2_keys):
    """rotateColumnsPow2(ct, generator, k, evakeyRotCol): pow2_keys = {2^i: key}"""
    steps = pow2_steps(N, generator, k)
    return chain(oplan, Q, ct, [g for g, _ in steps], [pow2_keys[i] for _, i in steps], False)
