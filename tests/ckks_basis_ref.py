"""Test helper (not a test module): the power basis of the reference's polynomial and Chebyshev evaluation -- computePowerBasis
(ckks/polynomial_evaluation.go:76-93), computePowerBasisCheby (ckks/chebyshev_evaluation.go:60-101) and the target lists of the four
Evaluate* entry points (:20-29, :46-55 and the monomial twins) -- restated in Python.

The scalar side (`schedule`) is the recursion on a dictionary, as the reference has it, MulRelinNew's level and scale (ckks/evaluator.go:
1005, :1038) and Rescale's loop (:938-961) on Python floats (one IEEE operation each), with ckks_combine_ref.constants for Sub's words and
ckks_lincomb_ref.half_words for AddConst's.  The element side (`Elements`) composes the oracle's mulrelin and its
DivRoundByLastModulusNTT with integer arithmetic for the tail: MRed on Python integers (ckks_lincomb_ref.mred), the CRed steps on rows
of 64-bit words, which hold every sum of two values at most q < 2^61 exactly.  Nothing of the library's C++ is imported."""
import math

import numpy as np

import ckks_combine_ref as combine_ref
from ckks_lincomb_ref import DomainError, half_words, mred

DEFAULT_SCALE = {"PN12QP109": 2.0 ** 32, "PN13QP218": 2.0 ** 30, "PN14QP438": 2.0 ** 34, "PN15QP880": 2.0 ** 40, "PN16QP1761": 2.0 ** 45}   # ckks/params.go:45-85


class Product:
    FIELDS = ("n", "a", "b", "c", "mul_level", "n_rescales", "level_after", "layer", "tail", "mult_side", "scale_after")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])
        self.mult = kw["mult"]       # [n_moduli] words, zero where unused
        self.add = kw["add"]

    def fields(self):
        return tuple(getattr(self, f) for f in self.FIELDS)


def targets(degree, fast):
    """the n of the computePowerBasis(Cheby) calls of Evaluate{Poly,Cheby}{Fast,Eco}, in order"""
    M = (degree - 1).bit_length()                     # bits.Len64(degree - 1)
    L = M >> 1 if fast else 1
    out = []
    i = 2
    while i <= (1 << L):                              # for i := uint64(2); i <= (1 << L); i++
        out.append(i)
        i += 1
    i = L + 1
    while i < M:                                      # for i := L + 1; i < M; i++
        out.append(1 << i)
        i += 1
    return out


def schedule(moduli, default_scale, chebyshev, c1_level, c1_scale, target_list):
    """[Product] in the order the reference creates them.  DomainError outside the domain the header states."""
    moduli = [int(q) for q in moduli]
    nm = len(moduli)
    if not 0 <= c1_level < nm:
        raise DomainError("a count or a level is out of range")
    if any(not 1 <= t <= 65535 for t in target_list):
        raise DomainError("a target is 0 or above 65535")
    if not all(math.isfinite(s) and s > 0 for s in (default_scale, c1_scale)):
        raise DomainError("a scale is not finite and positive")
    C = {1: (c1_level, float(c1_scale), 0)}           # n -> (level, scale, layer)
    out = []

    def compute(n):
        if n in C:                                    # if C[n] == nil
            return
        a = int(math.ceil(float(n) / 2))
        b = n >> 1
        c = int(abs(float(a) - float(b))) if chebyshev else 0
        compute(a)
        compute(b)
        if chebyshev and c != 0:
            compute(c)
        (la, sa, ya), (lb, sb, yb) = C[a], C[b]
        mul_level = min(la, lb)                       # MulRelinNew, :1005
        scale = sa * sb                               # :1038
        if not (math.isfinite(scale) and scale > 0):
            raise DomainError("a scale is not finite and positive")
        level, n_rescales = mul_level, 0              # Rescale, :938-961
        if level != 0 and scale >= (default_scale * float(moduli[level])) / 2:
            while scale >= (default_scale * float(moduli[level])) / 2 and level != 0:
                scale = scale / float(moduli[level])
                level -= 1
                n_rescales += 1
        mult, add, tail, side = [0] * nm, [0] * nm, 0, 0
        if chebyshev:
            # Add(C[n], C[n], C[n]) :92: equal scales, nothing multiplied, level and scale stay
            if c == 0:
                tail = 2                              # AddConst(C[n], -1, C[n]) :96
                for i in range(level + 1):
                    add[i] = half_words(-1.0, 0.0, scale, moduli[i], 0)[0]
            else:
                tail = 1                              # Sub(C[n], C[c], C[n]) :98
                lc, sc, _ = C[c]
                level, scale, _, side, words = combine_ref.constants(moduli, "SUB", (1, level, scale), (1, lc, sc), (1, level, scale), "a")
                if words is not None:
                    mult[:len(words)] = words
        C[n] = (level, scale, 1 + max(ya, yb))
        out.append(Product(n=n, a=a, b=b, c=c, mul_level=mul_level, n_rescales=n_rescales, level_after=level, layer=1 + max(ya, yb), tail=tail,
                           mult_side=side, scale_after=scale, mult=mult, add=add))

    for t in target_list:
        compute(t)
    return out


class Elements:
    """the element side per batch member: C[n] as [2][level + 1, N] arrays over the oracle's calls"""

    def __init__(self, oracle, N, Q, P, evk):
        self.oracle, self.N, self.Q = oracle, N, [int(q) for q in Q]
        self.plan = oracle.CkksPlan(oracle.Context(N, self.Q), oracle.Context(N, [int(p) for p in P]))
        self.evk = evk
        self._ctx = {}

    def _rescale(self, p):
        limbs = p.shape[0]
        if limbs not in self._ctx:
            self._ctx[limbs] = self.oracle.Context(self.N, self.Q[:limbs])
        return self._ctx[limbs].rescale_op("oc_div_round_by_last_modulus_ntt", p)

    def run(self, products, c1_level, c1):
        """c1: [2][>= c1_level + 1, N]; returns {n: [2][level_after + 1, N]}"""
        C = {1: [np.ascontiguousarray(c1[u][:c1_level + 1], dtype=np.uint64) for u in range(2)]}
        for P in products:
            L1 = P.mul_level + 1
            a, b = (np.stack([C[x][0][:L1], C[x][1][:L1]]) for x in (P.a, P.b))
            r = list(self.plan.mulrelin(P.mul_level, a, b, self.evk))
            for _ in range(P.n_rescales):
                r = [self._rescale(x) for x in r]
            assert r[0].shape[0] == P.level_after + 1
            if P.tail:
                for u in range(2):
                    for i in range(P.level_after + 1):
                        q = self.Q[i]
                        row = _cred(r[u][i] + r[u][i], q)                                                 # Add(C, C, C)
                        if P.tail == 1:
                            y = C[P.c][u][i]
                            if P.mult_side == 1:
                                row = _mred(row, P.mult[i], q)
                            if P.mult_side == 2:
                                y = _mred(y, P.mult[i], q)
                            row = _cred((row + np.uint64(q)) - y, q)                                      # Sub, ring/ring.go:70
                        elif u == 0:
                            row = _cred(row + np.uint64(P.add[i]), q)                                     # AddConst, value[0]
                        r[u][i] = row
            C[P.n] = r
        return C


def _cred(x, q):
    """CRed on a row of words: every sum here is of two values at most q < 2^61, so uint64 holds it exactly"""
    assert x.dtype == np.uint64
    return np.where(x >= np.uint64(q), x - np.uint64(q), x).astype(np.uint64)


def _mred(x, w, q):
    """MRed of every word of a row by one word, on Python integers (ckks_lincomb_ref.mred)"""
    return np.array([mred(int(v), int(w), q) for v in x], dtype=np.uint64)
