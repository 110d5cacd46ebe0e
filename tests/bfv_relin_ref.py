"""Test helper (not a test module): bfv.evaluator.Relinearize of every degree (bfv/evaluator.go:480-499) composed from the CPU oracle as it
stands -- oplan.bfv_switch_keys per degree, the highest first, and evaluator.Add as a literal CRed in numpy uint64: r = x + y;
r - q if r >= q else r (ring.CRed), so operands that are not canonical -- q, 2q - 1 -- give what the reference's loop gives.  One
ciphertext at a time: ct is [degree + 1, |Q|, N] uint64 in the coefficient domain, keys[k] = evakey.evakey[k] as [beta, 2, |Q| + |P|, N],
the key that switches from s^(k + 2)."""
import numpy as np


def cred(x, q):
    """ring.CRed on arrays: one conditional subtraction (x < 2^64 as the callers' sums are)"""
    return np.where(x >= q, x - q, x)


def add(a, b, Q):
    """Context.Add: CRed(a + b) per limb; a, b [|Q|, N] with sums below 2^64"""
    q = np.array([int(x) for x in Q], dtype=np.uint64)[:, None]
    return cred(np.asarray(a, dtype=np.uint64) + np.asarray(b, dtype=np.uint64), q)


def relinearize(oplan, Q, ct, keys):
    """(a0, a1) = (ct[0], ct[1]); for deg = degree .. 2: (p0, p1) = switchKeys(ct[deg], keys[deg - 2]); a_k = CRed(a_k + p_k)"""
    ct = np.asarray(ct, dtype=np.uint64)
    a0, a1 = ct[0].copy(), ct[1].copy()
    for deg in range(ct.shape[0] - 1, 1, -1):
        p0, p1 = oplan.bfv_switch_keys(ct[deg], keys[deg - 2])
        a0, a1 = add(a0, p0, Q), add(a1, p1, Q)
    return np.stack([a0, a1])
