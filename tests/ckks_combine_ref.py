"""Test helper (not a test module): evaluator.Add / AddNoMod / Sub / SubNoMod as the reference runs them -- getElemAndCheckBinary
(ckks/evaluator.go:112-126), evaluateInPlace (:227-342) with Resize (ckks/operand.go:68-80), DropLevel (:901-914) and the MultByConst
(:622-734) calls that equalise scales, into the evaluator's degree-1 pool ciphertext (:106) or in place, and Sub's NegLvl tail (:186-192,
:203-209) -- restated line by line on a small model of the reference's objects; then the Chebyshev step of computePowerBasisCheby
(ckks/chebyshev_evaluation.go:92-99) and the affine head of EvaluateChebyFast / Eco (:16-17) as sequences of those calls.

An Element is a ciphertext: `value`, one entry per component, each a list of limbs (the reference's Coeffs), `scale`.  A limb is either a
numpy row (with an oracle context: the element loops run, as oracle.ewise / oracle.half_scalar_op calls) or None (the scalar side only).
The 64-bit words are Python integers (ckks_lincomb_ref's MRed / MForm / CRed), the scales Python floats (one IEEE operation each);
nothing of the library's C++ is imported.  Where the reference panics, Panic is raised."""
import math

import numpy as np

from ckks_encoder_ref import scale_up_exact
from ckks_lincomb_ref import DomainError, TWO63, half_words, half_words_mform, mform

W = 1 << 64
OPS = ("ADD", "ADD_NOMOD", "SUB", "SUB_NOMOD")


class Panic(Exception):
    """the reference panics here"""


class Element:
    def __init__(self, degree, level, scale, N=None, data=None):
        """data: [degree + 1][level + 1, N] words, or None for limbs without contents"""
        self.scale = float(scale)
        if data is None:
            self.value = [[None if N is None else np.zeros(N, dtype=np.uint64) for _ in range(level + 1)] for _ in range(degree + 1)]
        else:
            self.value = [[np.array(row, dtype=np.uint64) for row in comp[:level + 1]] for comp in data]

    def degree(self):
        return len(self.value) - 1

    def level(self):
        return len(self.value[0]) - 1

    def array(self, u, level):
        return np.array([self.value[u][i] for i in range(level + 1)], dtype=np.uint64)


def _uint64_of(ratio):
    """uint64(ratio) inside the domain in which Go defines it the same on every machine"""
    if not (0 <= ratio < TWO63):
        raise DomainError("a scale ratio is not below 2^63")
    return math.trunc(ratio)


class Evaluator:
    """what evaluateInPlace needs of ckks.evaluator: the moduli, the pool ciphertext and, for the element loops, an oracle context"""

    def __init__(self, moduli, oc=None, default_scale=2.0 ** 40, psi1=None):
        self.moduli = [int(q) for q in moduli]
        self.oc = oc
        self.N = None if oc is None else oc.N
        self.default_scale = float(default_scale)
        self.psi1 = [0] * len(self.moduli) if psi1 is None else [int(p) for p in psi1]
        self.ctxpool = Element(1, len(self.moduli) - 1, default_scale, self.N)          # NewCiphertext(params, 1, MaxLevel, Scale), :106
        self.mults = []                       # every MultByConst that ran: (source, receiver, level, lo words, hi words)

    # ---- the ring's element loops on limbs 0 .. level ----
    def _ewise(self, op, level, a, b, out):
        if self.oc is None:
            return
        for i in range(level + 1):            # the limbs of out, a and b exist up to `level`, or Go's index runs out of range
            if a[i] is None or out[i] is None or (b is not None and b[i] is None):
                raise Panic("index out of range")
        x = np.array(a[:level + 1], dtype=np.uint64)
        y = None if b is None else np.array(b[:level + 1], dtype=np.uint64)
        r = self.oc.ewise(op, x, y, level=level)
        for i in range(level + 1):
            out[i][:] = r[i]

    # ---- ckks/evaluator.go ----
    def mult_by_const(self, ct0, constant, ct_out):                                     # :622-734
        level = min(ct0.level(), ct_out.level())                                        # :626
        if isinstance(constant, int):                                                   # case uint64, :669-671
            c_real, c_imag, scale = float(constant), 0.0, 1.0
        else:                                                                           # case complex128 / float64, :634-667
            c = complex(constant)
            c_real, c_imag = c.real, c.imag
            frac = lambda v: v != 0 and v - float(math.trunc(v)) != 0
            scale = self.default_scale if frac(c_real) or frac(c_imag) else 1.0
        words = [half_words_mform(c_real, c_imag, scale, q, psi) for q, psi in zip(self.moduli[:level + 1], self.psi1)]     # :688-709, :719-722
        lo, hi = [w[0] for w in words], [w[1] for w in words]
        for u in range(len(ct0.value)):                                                 # for u := range ct0.Value(), :711, :724
            if u >= len(ct_out.value):
                raise Panic("index out of range")                                       # ctOut.Value()[u], :713
            if self.oc is not None:
                r = self.oc.half_scalar_op(1, ct0.array(u, level), lo, hi)
                for i in range(level + 1):
                    ct_out.value[u][i][:] = r[i]
        self.mults.append((ct0, ct_out, level, lo, hi))
        ct_out.scale = ct0.scale * scale                                                # :733

    def add_const(self, ct0, constant, ct_out):                                         # :373-444
        level = min(ct0.level(), ct_out.level())
        c = complex(constant)
        words = [half_words(c.real, c.imag, ct0.scale, q, psi) for q, psi in zip(self.moduli[:level + 1], self.psi1)]
        lo, hi = [w[0] for w in words], [w[1] for w in words]
        if self.oc is not None:
            r = self.oc.half_scalar_op(0, ct0.array(0, level), lo, hi)
            for i in range(level + 1):
                ct_out.value[0][i][:] = r[i]
        return lo, hi

    def drop_level(self, ct0, levels):                                                  # :901-914
        if ct0.level() == 0:
            return "cannot DropLevel: Ciphertext already at level 0"                    # (evaluateInPlace ignores the error)
        keep = (ct0.level() + 1 - levels) % W                                           # uint64 arithmetic
        for comp in ct0.value:
            if keep > len(comp):
                raise Panic("slice bounds out of range")                                # Coeffs[:level+1-levels], :910
            del comp[keep:]
        return None

    def resize(self, el, degree):                                                       # ckks/operand.go:68-80
        if el.degree() > degree:
            del el.value[degree + 1:]
        while el.degree() < degree:
            el.value.append([None if self.N is None else np.zeros(self.N, dtype=np.uint64) for _ in range(el.level() + 1)])

    def check_binary(self, op0, op1, op_out, min_degree):                               # getElemAndCheckBinary, :112-126
        if op0.degree() + op1.degree() == 0:
            raise Panic("operands cannot be both plaintext")
        if op_out.degree() < min_degree:
            raise Panic("receiver operand degree is too small")

    def evaluate_in_place(self, c0, c1, ct_out, op):                                    # :227-342
        level = min(min(c0.level(), c1.level()), ct_out.level())                        # :231
        max_degree, min_degree = max(c0.degree(), c1.degree()), min(c0.degree(), c1.degree())
        self.resize(ct_out, max_degree)                                                 # :237
        self.drop_level(ct_out, (ct_out.level() - min(c0.level(), c1.level())) % W)     # :238
        if ct_out is c0:                                                                # :243
            if c0.scale > c1.scale:
                tmp1 = self.ctxpool
                if _uint64_of(c0.scale / c1.scale) != 0:
                    self.mult_by_const(c1, _uint64_of(c0.scale / c1.scale), tmp1)
            elif c1.scale > c0.scale:
                if _uint64_of(c1.scale / c0.scale) != 0:
                    self.mult_by_const(c0, _uint64_of(c1.scale / c0.scale), c0)
                c0.scale = c1.scale
                tmp1 = c1
            else:
                tmp1 = c1
            tmp0 = c0
        elif ct_out is c1:                                                              # :270
            if c1.scale > c0.scale:
                tmp0 = self.ctxpool
                if _uint64_of(c1.scale / c0.scale) != 0:
                    self.mult_by_const(c0, _uint64_of(c1.scale / c0.scale), tmp0)
            elif c0.scale > c1.scale:
                if _uint64_of(c0.scale / c1.scale) != 0:
                    self.mult_by_const(c1, _uint64_of(c0.scale / c1.scale), ct_out)
                ct_out.scale = c0.scale
                tmp0 = c0
            else:
                tmp0 = c0
            tmp1 = c1
        else:                                                                           # :296
            if c1.scale > c0.scale:
                tmp0 = self.ctxpool
                if _uint64_of(c1.scale / c0.scale) != 0:
                    self.mult_by_const(c0, _uint64_of(c1.scale / c0.scale), tmp0)
                tmp1 = c1
            elif c0.scale > c1.scale:
                tmp1 = self.ctxpool
                if _uint64_of(c0.scale / c1.scale) != 0:
                    self.mult_by_const(c1, _uint64_of(c0.scale / c1.scale), tmp1)
                tmp0 = c0
            else:
                tmp0, tmp1 = c0, c1
        for i in range(min_degree + 1):                                                 # :324-326
            self._ewise(op, level, tmp0.value[i], tmp1.value[i], ct_out.value[i])
        ct_out.scale = max(c0.scale, c1.scale)                                          # :328
        if c0.degree() > c1.degree() and tmp0 is not ct_out:                            # :333
            for i in range(min_degree + 1, max_degree + 1):
                self._ewise("COPY", level, tmp0.value[i], None, ct_out.value[i])
        elif c1.degree() > c0.degree() and tmp1 is not ct_out:                          # :337
            for i in range(min_degree + 1, max_degree + 1):
                self._ewise("COPY", level, tmp1.value[i], None, ct_out.value[i])

    def combine(self, op, op0, op1, ct_out):
        """Add (:154), AddNoMod (:160), Sub (:180), SubNoMod (:197)"""
        assert op in OPS
        self.check_binary(op0, op1, ct_out, max(op0.degree(), op1.degree()))
        self.evaluate_in_place(op0, op1, ct_out, op)
        if op in ("SUB", "SUB_NOMOD"):
            level = min(min(op0.level(), op1.level()), ct_out.level())                  # :186, :203
            if op0.degree() < op1.degree():
                for i in range(op0.degree() + 1, op1.degree() + 1):
                    self._ewise("NEG", level, ct_out.value[i], None, ct_out.value[i])   # :190, :207

    # ---- ckks/chebyshev_evaluation.go ----
    def chebyshev_step(self, cn, cc):
        """:92-99 after the product: C[n] = 2 C[n] - C[c], or 2 C[n] - 1 where c == 0 (cc None).  Returns AddConst's words or None."""
        self.combine("ADD", cn, cn, cn)                                                 # :92
        if cc is None:
            return self.add_const(cn, -1, cn)                                           # :96
        self.combine("SUB", cn, cc, cn)                                                 # :98
        return None

    def affine_head(self, c1, m, c):
        """:16-17 (:42-43): MultByConst(C[1], m, C[1]); AddConst(C[1], c, C[1]).  Returns AddConst's words."""
        self.mult_by_const(c1, float(m) if not isinstance(m, complex) else m, c1)
        return self.add_const(c1, float(c) if not isinstance(c, complex) else c, c1)


def constants(moduli, op, a, b, out, receiver):
    """The scalar side of one call: a, b, out = (degree, level, scale); receiver "new" | "a" | "b" | "both".  Runs the model without
    contents and reads off what it did: (level_after, scale_after, degree_after, mult_side, mult words or None).  Panic where the
    reference panics, DomainError outside the domain."""
    moduli = [int(q) for q in moduli]
    for d, l, s in (a, b, out):
        if not (0 <= d <= 2 and 0 <= l < len(moduli)):
            raise DomainError("a degree or a level is out of range")
        if not (math.isfinite(s) and s > 0):
            raise DomainError("a scale is not finite and positive")
    ev = Evaluator(moduli)
    ea = Element(*a)
    eb = ea if receiver == "both" else Element(*b)
    eo = {"new": None, "a": ea, "b": eb, "both": ea}[receiver] or Element(*out)
    ev.combine(op, ea, eb, eo)
    assert len(ev.mults) <= 1
    side, mult = 0, None
    if ev.mults:
        src, _, level, lo, hi = ev.mults[0]
        assert lo == hi and level >= eo.level()                                         # a real constant; every limb the element loops read
        side, mult = (1 if src is ea else 2), lo[:eo.level() + 1]
    return eo.level(), eo.scale, eo.degree(), side, mult


def ratio_word(r, q):
    """the per-limb word of MultByConst(ct, uint64 r, ...) written out once more, without the model: MForm(scaleUpExact(float64(r), 1, q))"""
    return mform(scale_up_exact(float(r), 1.0, q), q)


def elements(oc, op, level, a, b=None, double_a=False, ma=None, mb=None, add=None):
    """The element loops of one fused call as the sequence of oracle calls it replaces: ewise ADD of a with itself (double_a),
    half_scalar_op 1 on every component of a (ma) and of b (mb), the operation on the shared components, COPY of the surplus ones and NEG
    where they come from the subtrahend, half_scalar_op 0 on component 0 (add).  a, b: lists of arrays with at least level + 1 limbs (b
    None: no b); ma, mb, add: (lo, hi).  Returns the result's components, [level + 1, N] each; no argument is changed."""
    L1 = level + 1
    x = [np.ascontiguousarray(p[:L1], dtype=np.uint64) for p in a]
    y = [] if b is None else [np.ascontiguousarray(p[:L1], dtype=np.uint64) for p in b]
    if double_a:
        x = [oc.ewise("ADD", p, p) for p in x]
    if ma is not None:
        x = [oc.half_scalar_op(1, p, ma[0][:L1], ma[1][:L1]) for p in x]
    if mb is not None:
        y = [oc.half_scalar_op(1, p, mb[0][:L1], mb[1][:L1]) for p in y]
    res = []
    for u in range(max(len(x), len(y))):
        if u < len(x) and u < len(y):
            r = oc.ewise(op, x[u], y[u])
        elif u < len(x):
            r = oc.ewise("COPY", x[u])
        else:
            r = oc.ewise("COPY", y[u])
            if op in ("SUB", "SUB_NOMOD"):
                r = oc.ewise("NEG", r)
        res.append(r)
    if add is not None:
        res[0] = oc.half_scalar_op(0, res[0], add[0][:L1], add[1][:L1])
    return res
