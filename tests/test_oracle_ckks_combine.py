"""lr_ckks_combine_constants (the scalar side of evaluator.Add / AddNoMod / Sub / SubNoMod, host only: no device is needed) against the
line-by-line restatement of getElemAndCheckBinary, evaluateInPlace, Resize, DropLevel and MultByConst in tests/ckks_combine_ref.py, word
for word, over the whole grid of operations, degree pairs, receiver identities, scale ratios on either side and level mixes; where the
restatement panics the call answers LR_ERR_UNSUPPORTED; every refusal by message, with nothing written.  CPU only.

The ratio "just below 2^63" is 2^63 - 2^10: uint64(ratio) lies above 2^53 there, and MultByConst converts it back to a float64 (:670).
The quotient of two doubles is a double, so above 2^53 it is an integer that the round trip returns unchanged; what rounds at that size
is scaleUpExact's + 0.5 (ties to even), which the restatement and the library both carry."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ckks_combine_ref as ref
import limit_moduli as lm

LOGN = 4
ARG, UNSUPPORTED = 4, 6
DEGREES = [(0, 1), (1, 0), (1, 1), (2, 1), (1, 2), (2, 2)]
RECEIVERS = ["new", "a", "b", "both"]
RATIOS = [1.0, 1.5, 2.0, 2.0 ** 20 + 0.75, 2.0 ** 63 - 2.0 ** 10]
BASE = 2.0 ** 24                     # the smaller scale: every ratio times it is exact, so larger / smaller gives the ratio back


def _moduli():
    """next to 2^61 from below (the admission bound), 2^60 from either side, a CKKS-size prime and the 14-bit 12289"""
    return [lm.below(61, LOGN), lm.below(61, LOGN, 2)[1], lm.above(60, LOGN), lm.below(60, LOGN), lm.below(46, LOGN), 12289]


def _levels(receiver, top):
    """(a, b, out) levels: equal, mixed, the receiver above the operands, at level 0, and above 0 below both (the reference panics)"""
    if receiver == "both":
        return [(top, top, top), (0, 0, 0)]
    if receiver == "a":
        return [(top, top, top), (2, 3, 2), (3, 1, 3), (0, 2, 0)]
    if receiver == "b":
        return [(top, top, top), (2, 3, 3), (3, 1, 1), (2, 0, 0)]
    return [(top, top, top), (2, 1, 3), (1, 2, top), (2, 3, 0), (2, 3, 1), (3, 3, 2), (1, 2, 1)]


def _compare(pkg, moduli, op, a, b, out, receiver):
    """the library against the restatement: the same result word for word, or the refusal that stands for the reference's panic"""
    try:
        want = ref.constants(moduli, op, a, b, out, receiver)
    except ref.Panic as p:
        with pytest.raises(pkg.ring.LatticeRingError) as e:
            pkg.ring.ckks_combine_constants(moduli, op, a, b, out, receiver)
        assert e.value.code == UNSUPPORTED, (op, a, b, out, receiver, str(p), str(e.value))
        return ("panic", str(p), str(e.value))
    got = pkg.ring.ckks_combine_constants(moduli, op, a, b, out, receiver)
    level, scale, degree, side, mult = want
    assert (got.level_after, got.scale_after, got.degree_after, got.mult_side) == (level, scale, degree, side), (op, a, b, out, receiver)
    if side == 0:
        assert got.mult is None and mult is None
    else:
        assert [int(v) for v in got.mult] == mult, (op, a, b, out, receiver)
    return want


@pytest.mark.parametrize("op", ref.OPS)
def test_the_grid_word_for_word(pkg, op):
    moduli = _moduli()
    top = len(moduli) - 1
    seen = {"panic": set(), "side": set(), "results": 0}
    for (da, db), receiver, ratio, a_larger in itertools.product(DEGREES, RECEIVERS, RATIOS, (False, True)):
        if receiver == "both" and (da != db or ratio != 1.0):
            continue                                         # a is b: one degree, one scale
        if ratio == 1.0 and a_larger:
            continue
        sa, sb = (BASE * ratio, BASE) if a_larger else (BASE, BASE * ratio)
        assert max(sa, sb) / min(sa, sb) == ratio
        for la, lb, lo in _levels(receiver, top):
            a, b = (da, la, sa), (db, lb, sb)
            outs = {"a": [a], "b": [b], "both": [a]}.get(receiver) or [(d, lo, BASE * 3) for d in sorted({max(da, db), 2, max(da, db) - 1})]
            for out in outs:
                r = _compare(pkg, moduli, op, a, b, out, receiver)
                if r[0] == "panic":
                    seen["panic"].add(r[2])
                    continue
                seen["results"] += 1
                level, scale, degree, side, mult = r
                seen["side"].add((receiver, side))
                # what the lines say, once more without the model
                assert level == min(la, lb, out[1]) and scale == max(sa, sb) and degree == max(da, db)
                assert side == (0 if ratio == 1.0 else 2 if a_larger else 1)
                if side:
                    word = int(ratio)                        # truncated: 1.5 multiplies by 1, and the multiplication takes place
                    assert mult == [ref.ratio_word(word, q) for q in moduli[:level + 1]]
                    if word < 1 << 53:
                        assert mult == [word * (1 << 64) % q for q in moduli[:level + 1]]
    # every refusal that stands for a panic was reached (a degree-0 pair is not in the grid: below), every side with every receiver
    who = "LR_ERR_UNSUPPORTED: CKKS combine constants: "
    assert seen["panic"] == {who + m for m in ("the receiver's degree is below the larger operand degree",
                                               "the receiver lies above level 0 and below both operand levels",
                                               "the operand to be multiplied has degree 2 and is not the receiver")}
    assert seen["side"] == {(r, s) for r in ("new", "a", "b") for s in (0, 1, 2)} | {("both", 0)}
    assert seen["results"] > 300


def test_a_multiplied_operand_of_degree_2_only_as_the_receiver(pkg):
    """MultByConst into the pool ciphertext of degree 1 panics at the third component; in place on the receiver it does not"""
    moduli = _moduli()
    top = len(moduli) - 1
    small, large = (2, top, BASE), (1, top, BASE * 4)
    for op in ref.OPS:
        for a, b, side_name in ((small, large, "a"), (large, small, "b")):
            for receiver in ("new", side_name):            # (the other operand as the receiver has too small a degree)
                out = {"a": a, "b": b}.get(receiver, (2, top, BASE))
                r = _compare(pkg, moduli, op, a, b, out, receiver)
                if receiver == side_name:
                    assert r[3] == (1 if side_name == "a" else 2) and r[4] == [4 * (1 << 64) % q for q in moduli]
                else:
                    assert r[0] == "panic" and r[1] == "index out of range" and r[2].endswith("has degree 2 and is not the receiver")


def _raw(pkg, moduli, op, a, b, out, receiver, n_moduli=None, nulls=()):
    """lr_ckks_combine_constants itself with sentinels in every output; returns (status, message, outputs untouched?)"""
    lib = pkg._native.lib()
    m = (C.c_uint64 * len(moduli))(*moduli)
    la, da, ms = C.c_int(-7), C.c_int(-7), C.c_int(-7)
    sa = C.c_double(-7.0)
    mult = np.full(len(moduli), 7, dtype=np.uint64)
    args = {"moduli": m, "level_after": C.byref(la), "scale_after": C.byref(sa), "degree_after": C.byref(da), "mult_side": C.byref(ms),
            "mult": mult.ctypes.data_as(C.c_void_p)}
    for n in nulls:
        args[n] = None
    rc = lib.lr_ckks_combine_constants(args["moduli"], len(moduli) if n_moduli is None else n_moduli, op, a[0], a[1], a[2], b[0], b[1], b[2], out[0],
                                       out[1], out[2], receiver, args["level_after"], args["scale_after"], args["degree_after"], args["mult_side"],
                                       args["mult"])
    untouched = (la.value, da.value, ms.value, sa.value) == (-7, -7, -7, -7.0) and bool(np.all(mult == 7))
    return rc, lib.lr_last_error_string().decode(), untouched


def test_every_refusal_by_message_with_nothing_written(pkg):
    moduli = _moduli()
    top = len(moduli) - 1
    s = BASE
    a, b, out = (1, top, s), (1, top, s * 2), (1, top, s)
    who = "CKKS combine constants: "
    inf, nan = float("inf"), float("nan")
    cases = [
        # LR_ERR_ARG, in the order of the contract
        (dict(nulls=("moduli",)), ARG, "null argument"), (dict(nulls=("level_after",)), ARG, "null argument"),
        (dict(nulls=("scale_after",)), ARG, "null argument"), (dict(nulls=("degree_after",)), ARG, "null argument"),
        (dict(nulls=("mult_side",)), ARG, "null argument"), (dict(nulls=("mult",)), ARG, "null argument"),
        (dict(n_moduli=0), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(op=4), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(op=-1), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(receiver=4), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(a=(3, top, s)), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(b=(-1, top, s)), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(out=(1, top + 1, s)), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(a=(1, -1, s)), ARG, "a count, the operation, the receiver, a degree or a level is out of range"),
        (dict(moduli=moduli[:2] + [moduli[2] + 1] + moduli[3:]), ARG, "a modulus is even, below 3 or not below 2^61"),
        (dict(moduli=moduli[:2] + [1] + moduli[3:]), ARG, "a modulus is even, below 3 or not below 2^61"),
        (dict(moduli=moduli[:2] + [lm.above(61, LOGN)] + moduli[3:]), ARG, "a modulus is even, below 3 or not below 2^61"),
        (dict(a=(1, top, 0.0)), ARG, "a scale is not finite and positive"), (dict(b=(1, top, -s)), ARG, "a scale is not finite and positive"),
        (dict(a=(1, top, inf)), ARG, "a scale is not finite and positive"), (dict(out=(1, top, nan)), ARG, "a scale is not finite and positive"),
        (dict(receiver=1, out=(2, top, s)), ARG, "the receiver is an operand and differs from it in degree, level or scale"),
        (dict(receiver=2, out=(1, top, s)), ARG, "the receiver is an operand and differs from it in degree, level or scale"),
        (dict(receiver=3, out=(1, top, s)), ARG, "the receiver is an operand and differs from it in degree, level or scale"),
        (dict(b=(1, top, s * 2.0 ** 63)), ARG, "a scale ratio is not below 2^63"),
        (dict(a=(1, top, 1e300), b=(1, top, 1e-300), out=(1, top, 1.0)), ARG, "a scale ratio is not below 2^63"),      # the quotient is infinite
        # the domain before the panics
        (dict(a=(0, top, s), b=(0, top, s * 2.0 ** 63)), ARG, "a scale ratio is not below 2^63"),
        # LR_ERR_UNSUPPORTED: the reference's panics, in the order it meets them
        (dict(a=(0, top, s), b=(0, top, s)), UNSUPPORTED, "both operands have degree 0"),
        (dict(a=(0, top, s), b=(0, top, s), out=(0, 1, s)), UNSUPPORTED, "both operands have degree 0"),
        (dict(b=(2, 3, s), out=(1, 1, s)), UNSUPPORTED, "the receiver's degree is below the larger operand degree"),
        (dict(a=(1, 3, s), b=(2, 2, s), out=(2, 1, s)), UNSUPPORTED, "the receiver lies above level 0 and below both operand levels"),
        (dict(a=(2, top, s), b=(1, top, s * 2), out=(2, top, s)), UNSUPPORTED, "the operand to be multiplied has degree 2 and is not the receiver"),
    ]
    base = dict(moduli=moduli, op=0, a=a, b=b, out=out, receiver=0)
    for change, code, message in cases:
        rc, msg, untouched = _raw(pkg, **dict(base, **change))
        assert (rc, msg) == (code, who + message), (change, rc, msg)
        assert untouched, change
    rc, _, untouched = _raw(pkg, **base)                   # the same arguments unchanged are accepted
    assert rc == 0 and not untouched


def test_the_ratio_guards_cannot_fail(pkg):
    """`uint64(ratio) != 0` (:249 ...) holds for every pair of finite positive scales: the correctly rounded quotient of x > y > 0 is at
    least 1.  The smallest ratios there are, on the restatement and on the library: the word is 1 and the operand is still multiplied."""
    moduli = _moduli()
    top = len(moduli) - 1
    for small in (1.0, BASE, 2.2250738585072014e-308, 1.7976931348623155e308):     # (normal numbers: one step up is a ratio below 2)
        large = np.nextafter(small, np.inf)
        assert large / small >= 1
        for a, b, side in (((1, top, small), (1, top, float(large)), 1), ((1, top, float(large)), (1, top, small), 2)):
            r = _compare(pkg, moduli, "ADD", a, b, (1, top, 1.0), "new")
            assert r[3] == side and r[4] == [(1 << 64) % q for q in moduli]
