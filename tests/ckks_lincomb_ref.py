"""Test helper (not a test module): res = c0 + sum c_k ct_k as the reference runs it -- evaluatePolyFromPowerBasis' chain (ckks/
polynomial_evaluation.go:142-159) of one AddConst (ckks/evaluator.go:373-444) and per term MultByConstAndAdd (:451-608), with the
MultByConst (:622-734) calls on the receiver that it makes at :530 and :553 -- restated line by line in the caller's order.

The scalar side (`constants`) is written with Python integers for the 64-bit words (MRed, MForm and CRed spelled out on integers with
their wrap-arounds), Python floats where the reference has float64 (a Python float operation is one IEEE operation), `fractions` for the
questions that are about exact values (does a constant have a fractional part), and ckks_encoder_ref.scale_up_exact for the rounding of
scaleUpExact; nothing of the library's C++ is imported.  The element side (`elements`) is the sequence of oracle.half_scalar_op calls."""
import math
from fractions import Fraction

import numpy as np

from ckks_encoder_ref import scale_up_exact

W = 1 << 64
TWO63 = float(1 << 63)


class DomainError(ValueError):
    """outside the domain in which Go's float-to-integer conversions are defined the same on every machine"""


def cred(a, q):                                   # ring/modular_reduction.go:211
    return a - q if a >= q else a


def mred(x, y, q):                                # :70, with MRedParams (:53) = q^-1 mod 2^64
    ahi, alo = divmod(x * y, W)
    h = (((alo * pow(q, -1, W)) % W) * q) >> 64
    return cred((ahi - h + q) % W, q)


def mform(a, q):                                  # :15, with BRedParams (:97) = the two words of floor(2^128 / q)
    u0, u1 = divmod((1 << 128) // q, W)
    mhi = (a * u1) >> 64
    return cred(((-(a * u0 + mhi)) % W) * q % W, q)


def has_fraction(v):
    """:472-478: valueInt := int64(v); v - float64(valueInt) != 0 -- for |v| < 2^63 the truncation is exact, so: v is no integer"""
    return v != 0 and Fraction(v).denominator != 1


def _finite(*vals):
    return all(math.isfinite(v) for v in vals)


def _scaled(v, scale, q):
    if not math.isfinite(scale * v):
        raise DomainError("a constant times its scale is not finite")
    return scale_up_exact(v, scale, q)


def half_words(re, im, scale, q, psi):
    """scaledConst for the coefficients below and above N / 2, before any MForm (:413-427 and :436-438; :570-583 and :595-596)"""
    sc = sc_real = sc_imag = 0
    if re != 0:
        sc_real = _scaled(re, scale, q)
        sc = sc_real
    if im != 0:
        sc_imag = mred(_scaled(im, scale, q), psi, q)
        sc = cred(sc + sc_imag, q)
    lo = sc
    if im != 0:
        sc = cred(sc_real + (q - sc_imag), q)
    return lo, sc


def half_words_mform(re, im, scale, q, psi):
    lo, hi = half_words(re, im, scale, q, psi)
    lo = mform(lo, q)                              # :585
    return lo, (mform(hi, q) if im != 0 else lo)   # :595-598


def _ratio_word(ratio):
    """uint64(ratio) inside the domain"""
    if not (0 <= ratio < TWO63):
        raise DomainError("a scale ratio is not below 2^63")
    return math.trunc(ratio)


class Consts:
    def __init__(self):
        self.level_after = self.scale_after = None
        self.add = None                            # ([level_after + 1], [level_after + 1]) with a constant term
        self.has_pre, self.pre, self.lo, self.hi = [], [], [], []
        self.quirk = []                            # per term: did :553 scale its ratio by the default scale


def constants(moduli, psi1, default_scale, res_level, res_scale, terms, c0=None):
    """terms: [(constant, scale, level), ...] in the order of the chain; c0: None or the constant of AddConst.  Words for the limbs
    0 .. level_after (DropLevel, :457-460, only lowers the level: what a step computes for a limb does not depend on the limbs above it)."""
    moduli = [int(q) for q in moduli]
    terms = [(complex(c), float(s), int(l)) for c, s, l in terms]
    delta, scale_out = float(default_scale), float(res_scale)
    if not all(0 <= l < len(moduli) for l in [res_level] + [t[2] for t in terms]):
        raise DomainError("a count or a level is out of range")
    if not all(_finite(s) and s > 0 for s in [delta, scale_out] + [t[1] for t in terms]):
        raise DomainError("a scale is not finite and positive")
    for c in ([complex(c0)] if c0 is not None else []) + [t[0] for t in terms]:
        if not (_finite(c.real, c.imag) and abs(c.real) < TWO63 and abs(c.imag) < TWO63):
            raise DomainError("a constant is not finite and below 2^63 in magnitude")
    out = Consts()
    level = min([res_level] + [t[2] for t in terms])
    limbs = list(zip(moduli[:level + 1], [int(p) for p in psi1[:level + 1]]))
    if c0 is not None:                                                                         # AddConst(res, c0, res)
        c0 = complex(c0)
        words = [half_words(c0.real, c0.imag, scale_out, q, psi) for q, psi in limbs]
        out.add = ([w[0] for w in words], [w[1] for w in words])
    for c, ct_scale, _ in terms:                                                               # MultByConstAndAdd(ct, c, res)
        re, im = c.real, c.imag
        scale = delta if has_fraction(re) or has_fraction(im) else 1.0                         # :466-488
        pre, quirk = None, False
        if scale != 1:                                                                         # :522
            if scale_out < ct_scale * delta:                                                   # :526
                r = _ratio_word((delta * ct_scale) / scale_out)
                if r != 0:                                                                     # :528, :530: MultByConst with a uint64
                    pre = [half_words_mform(float(r), 0.0, 1.0, q, psi)[0] for q, psi in limbs]
                scale_out = delta * ct_scale                                                   # :534
            elif scale_out > ct_scale * delta:                                                 # :538
                scale = scale_out / ct_scale
        else:
            if scale_out > ct_scale:                                                           # :546
                scale = scale_out / ct_scale
            elif ct_scale > scale_out:                                                         # :550
                ratio = ct_scale / scale_out
                if _ratio_word(ratio) != 0:                                                    # :552, :553: MultByConst with a float64
                    quirk = has_fraction(ratio)
                    pre = [half_words_mform(ratio, 0.0, delta if quirk else 1.0, q, psi)[0] for q, psi in limbs]
                scale_out = ct_scale                                                           # :556
        words = [half_words_mform(re, im, scale, q, psi) for q, psi in limbs]
        out.has_pre.append(0 if pre is None else 1)
        out.pre.append([0] * (level + 1) if pre is None else pre)
        out.lo.append([w[0] for w in words])
        out.hi.append([w[1] for w in words])
        out.quirk.append(quirk)
    out.level_after, out.scale_after = level, scale_out
    return out


def elements(oc, level, terms, has_pre, pre, lo, hi, add=None, start=None):
    """The element loops as oracle.half_scalar_op calls: op 0 on component 0 with a constant term, then per term op 1 on the receiver
    where has_pre, and op 2.  terms: [(c0, c1), ...] arrays of at least level + 1 limbs; start: the receiver to accumulate on, or None
    for zeros.  Returns (res0, res1), [level + 1, N] each; no argument is changed."""
    L1 = level + 1
    res = []
    for u in range(2):
        acc = np.zeros((L1, oc.N), dtype=np.uint64) if start is None else np.array(start[u][:L1], dtype=np.uint64)
        if add is not None and u == 0:
            acc = oc.half_scalar_op(0, acc, add[0][:L1], add[1][:L1])
        for k, t in enumerate(terms):
            if has_pre[k]:
                acc = oc.half_scalar_op(1, acc, pre[k][:L1], pre[k][:L1])
            acc = oc.half_scalar_op(2, np.ascontiguousarray(t[u][:L1]), lo[k][:L1], hi[k][:L1], out=acc)
        res.append(acc)
    return res[0], res[1]
