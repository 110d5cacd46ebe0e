"""Test helper (not a test module): bfv tensorAndRescale (bfv/evaluator.go:278-464), every branch, restated line by line from the oracle's
ring primitives -- Context.ntt / intt / ewise and the BasisExtender's ModUpSplitQP / ModDownSplitedQP / ModUpSplitPQ.  oracle/ restates the
degree-1 branches only (oc_bfv_mul, oc_bfv_square); the branch for operands that are not both of degree 1 (:371-415) lives here."""
import numpy as np


def tensor_and_rescale(plan, ct0, ct1, square=False, out_degree=None):
    """plan: oracle.BfvPlan (contexts over Q and QMul, baseconverterQ1Q2, t, pHalf).  ct0 / ct1: sequences of [|Q|, N] polys over Q in the
    coefficient domain (a Plaintext is a sequence of one).  square: Go's `ct0 == ct1` (the operands are the same element; ct1 is then
    ignored).  out_degree: the receiver's degree (default d0 + d1).  Returns [out_degree + 1, |Q|, N]."""
    cQ, cM, bx = plan.cQ, plan.cM, plan.bext
    lQ, lM = cQ.L - 1, cM.L - 1
    ct0 = [np.ascontiguousarray(p, dtype=np.uint64) for p in ct0]
    ct1 = ct0 if square else [np.ascontiguousarray(p, dtype=np.uint64) for p in ct1]
    d0, d1 = len(ct0) - 1, len(ct1) - 1
    dout = d0 + d1 if out_degree is None else out_degree

    # :298-313  ModUpSplitQP, then NTT over Q and over QMul, for every poly of ct0 and (ct0 != ct1) of ct1
    def lift(p):
        q2 = bx.modup_split_qp(lQ, p)
        return cQ.ntt(p), cM.ntt(q2)

    c0Q1, c0Q2 = [list(x) for x in zip(*[lift(p) for p in ct0])]
    if square:
        c1Q1, c1Q2 = c0Q1, c0Q2
    else:
        c1Q1, c1Q2 = [list(x) for x in zip(*[lift(p) for p in ct1])]

    def both(op, a, b=None, out=None):
        """the same Context call over Q (index 0) and QMul (index 1)"""
        return (cQ.ewise(op, a[0], None if b is None else b[0], out=None if out is None else out[0]),
                cM.ewise(op, a[1], None if b is None else b[1], out=None if out is None else out[1]))

    a = [(c0Q1[i], c0Q2[i]) for i in range(d0 + 1)]
    b = [(c1Q1[j], c1Q2[j]) for j in range(d1 + 1)]
    if d0 == 1 and d1 == 1:
        # :320-369
        c00, c01 = both("MFORM", a[0]), both("MFORM", a[1])
        c2 = [None] * 3
        if square:
            c2[0] = both("MUL_MONT", c00, a[0])                                 # :337-338
            c2[1] = both("MUL_MONT", c00, a[1])                                 # :341-342
            c2[1] = both("ADD_NOMOD", c2[1], c2[1])                             # :344-345
            c2[2] = both("MUL_MONT", c01, a[1])                                 # :348-349
        else:
            c2[0] = both("MUL_MONT", c00, b[0])                                 # :355-356
            c2[1] = both("MUL_MONT", c00, b[1])                                 # :359-360
            c2[1] = both("MUL_MONT_AND_ADD_NOMOD", c01, b[0], out=c2[1])        # :362-363
            c2[2] = both("MUL_MONT", c01, b[1])                                 # :366-367
        c2 += [(np.zeros_like(c0Q1[0]), np.zeros_like(c0Q2[0]))] * (dout + 1 - 3)
    else:
        # :371-415
        c2 = [(np.zeros_like(c0Q1[0]), np.zeros_like(c0Q2[0])) for _ in range(dout + 1)]     # :373-376
        if square:
            m = [both("MFORM", a[i]) for i in range(d0 + 1)]                    # :385-386
            for i in range(d0 + 1):                                             # :389-396
                for j in range(i + 1, d0 + 1):
                    c2[i + j] = both("MUL_MONT", m[i], a[j])
                    c2[i + j] = both("ADD", c2[i + j], c2[i + j])
            for i in range(d0 + 1):                                             # :398-401
                c2[i << 1] = both("MUL_MONT_AND_ADD", m[i], a[i], out=c2[i << 1])
        else:
            for i in range(d0 + 1):                                             # :405-413
                mi = both("MFORM", a[i])
                for j in range(d1 + 1):
                    c2[i + j] = both("MUL_MONT_AND_ADD", mi, b[j], out=c2[i + j])

    # :417-463
    pq = np.array([plan.p_half % q for q in cQ.moduli], dtype=np.uint64)
    pm = np.array([plan.p_half % q for q in cM.moduli], dtype=np.uint64)
    out = np.zeros((dout + 1, cQ.L, cQ.N), dtype=np.uint64)
    for i in range(dout + 1):
        q1, q2 = cQ.intt(c2[i][0]), cM.intt(c2[i][1])                           # :424-425
        q2 = bx.moddown_split_qp(lQ, lM, q1, q2)                                # :450
        q2 = cM.ewise("ADD_SCALAR_LIMBS", q2, scalars=pm)                       # :457
        o = bx.modup_split_pq(lM, q2)                                           # :458
        o = cQ.ewise("SUB_SCALAR_LIMBS", o, scalars=pq)                         # :459
        out[i] = cQ.ewise("MUL_SCALAR", o, scalars=[plan.t])                    # :462
    return out


# -- encryption / decryption with Python integers (the arbiter of the algebra; the oracle supplies NTTs only) ---------------------
def prod(moduli):
    p = 1
    for q in moduli:
        p *= int(q)
    return p


def small(N, bound, seed):
    return np.random.default_rng(seed).integers(-bound, bound + 1, size=N)


def residues(v, moduli):
    return np.array([[int(x) % int(q) for x in v] for q in moduli], dtype=np.uint64)


def _mul(a, b, moduli):
    return np.array([(a[i].astype(object) * b[i].astype(object)) % int(q) for i, q in enumerate(moduli)], dtype=np.uint64)


def _add(a, b, moduli):
    return np.array([(a[i].astype(object) + b[i].astype(object)) % int(q) for i, q in enumerate(moduli)], dtype=np.uint64)


def uniform(moduli, N, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, int(q), size=N, dtype=np.uint64) for q in moduli])


def encode(moduli, t, m):
    """encodePlaintext (bfv/encoder.go:121-137): the message times deltaMont = floor(Q/t) (GenLiftParams), one poly over Q"""
    delta = prod(moduli) // t
    return residues([delta * int(x) for x in m], moduli)


def encrypt(ocQ, t, s, m, seed):
    """(b, a) with b = -a*s + floor(Q/t)*m + e, coefficient domain over Q; s and e small"""
    Q = ocQ.moduli
    a = uniform(Q, ocQ.N, seed)
    as_ = ocQ.intt(_mul(ocQ.ntt(a), ocQ.ntt(residues(s, Q)), Q))
    neg = np.array([(int(q) - as_[i].astype(object)) % int(q) for i, q in enumerate(Q)], dtype=np.uint64)
    body = _add(encode(Q, t, m), residues(small(ocQ.N, 6, seed + 1), Q), Q)
    return [_add(neg, body, Q), a]


def decrypt(ocQ, t, ct, s):
    """round(t/Q * sum_i ct[i] s^i) mod t, coefficient by coefficient"""
    Q = ocQ.moduli
    s_ntt = ocQ.ntt(residues(s, Q))
    acc, sp = None, None
    for i, c in enumerate(ct):
        term = ocQ.ntt(np.ascontiguousarray(c, dtype=np.uint64))
        if i:
            sp = s_ntt if sp is None else _mul(sp, s_ntt, Q)
            term = _mul(term, sp, Q)
        acc = term if acc is None else _add(acc, term, Q)
    v = ocQ.intt(acc)
    Qp = prod(Q)
    crt = [(Qp // int(q)) * pow(Qp // int(q), -1, int(q)) for q in Q]
    x = sum(v[i].astype(object) * crt[i] for i in range(len(Q))) % Qp
    return [int(((t * int(y) + Qp // 2) // Qp) % t) for y in x]


def negacyclic(m0, m1, t):
    """m0 * m1 mod (X^N + 1, t) for messages in [0, t) (t < 2^17: the int64 convolution does not overflow below N = 2^15)"""
    N = len(m0)
    full = np.convolve(np.asarray(m0, dtype=np.int64), np.asarray(m1, dtype=np.int64))
    out = full[:N].copy()
    out[:N - 1] -= full[N:]
    return [int(x) % t for x in out]
