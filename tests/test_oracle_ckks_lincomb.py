"""lr_ckks_lincomb_constants (the scalar side of res = c0 + sum c_k ct_k, host only: no device is needed) against the line-by-line
restatement of the reference's chain in tests/ckks_lincomb_ref.py, word for word, on cases that reach every branch of AddConst,
MultByConstAndAdd and the MultByConst calls it makes; every domain refusal, with nothing written; and what the restated chain MEANS:
on encoded slot vectors it computes c0 + sum c_k v_k within the precision the reference's own test demands.  CPU only.

One case of the issue's list cannot be built: "a ratio that truncates to 0".  The reference converts uint64(x / y) only under x > y > 0
(:526 / :528 with x = scale * ct.scale in either order of the same IEEE product, :550 / :552), and a correctly rounded quotient of
x > y > 0 is at least 1 (1 is a double and the exact quotient exceeds it), so `!= 0` at :528 and :552 always holds for finite positive
scales.  The smallest reachable word, 1 for a ratio in [1, 2) (the truncating equalisation), is covered instead, and
test_a_ratio_never_truncates_to_zero pins the argument on the restatement."""
import ctypes as C
import math

import numpy as np
import pytest

import ckks_encoder_ref as enc_ref
import ckks_lincomb_ref as ref
import limit_moduli as lm

DELTA = 2.0 ** 40
LOGN = 4


def _sets(pkg):
    """name -> moduli, all NTT-friendly at N = 2^LOGN: the 60-bit ring primes, CKKS-size primes (50 and 40 bits), and one limb per size
    class next to the admission bounds (tests/limit_moduli.py) with the 14-bit 12289"""
    return {"qi60": list(pkg.params.Qi60()[:4]), "ckks": list(pkg.params.ckks_moduli("PN15QP880")[1][:4]), "limit": lm.ewise_moduli(LOGN)[:6]}


_PSI = {}


def _psi1(oracle, moduli):
    key = tuple(moduli)
    if key not in _PSI:
        _PSI[key] = [int(v) for v in oracle.Context(1 << LOGN, moduli).ntt_psi[:, 1]]
    return _PSI[key]


def _check(pkg, oracle, moduli, res_level, res_scale, terms, c0=None, delta=DELTA):
    """the library's words against the restatement's, all of them; returns the restatement's result"""
    psi = _psi1(oracle, moduli)
    want = ref.constants(moduli, psi, delta, res_level, res_scale, terms, c0)
    got = pkg.ring.ckks_lincomb_constants(moduli, psi, delta, res_level, res_scale, terms, c0)
    assert got.level_after == want.level_after and got.scale_after == want.scale_after
    L1 = want.level_after + 1
    if c0 is None:
        assert got.add is None and want.add is None
    else:
        assert [int(v) for v in got.add[0]] == want.add[0] and [int(v) for v in got.add[1]] == want.add[1]
    assert [int(v) for v in got.has_pre] == want.has_pre
    for name in ("pre", "lo", "hi"):
        g = getattr(got, name)
        assert g.shape == (len(terms), L1)
        assert [[int(v) for v in row] for row in g] == getattr(want, name), name
    return want


def test_words_are_montgomery_forms_of_the_scaled_constants(pkg, oracle):
    """what the restatement's integer spellings of MRed and MForm mean, against plain modular arithmetic and the oracle's own"""
    for q in _sets(pkg)["limit"] + _sets(pkg)["ckks"]:
        R = 1 << 64
        for a in (0, 1, 2, q // 2, q - 1):
            assert ref.mform(a, q) == a * R % q == oracle.mform(a, q)
            for b in (1, q // 3, q - 1, q):
                assert ref.mred(b, a, q) == b * a * pow(R, -1, q) % q == oracle.mred(b, a, q)
        assert ref.mform(q, q) == oracle.mform(q, q)            # the word a negative multiple of q leaves (below)


@pytest.mark.parametrize("name", ["qi60", "ckks", "limit"])
def test_every_branch_of_the_chain(pkg, oracle, name):
    moduli = _sets(pkg)[name]
    top = len(moduli) - 1
    frac, whole = 0.5 - 0.25j, 3 + 2j
    s = DELTA
    # --- MultByConstAndAdd with a fractional constant (:522): the receiver's scale below, equal to and above ct.scale * Delta
    w = _check(pkg, oracle, moduli, top, s, [(frac, s, top)])
    assert w.has_pre == [1] and w.scale_after == DELTA * s and w.pre[0] == [ref.mform(int(DELTA) % q, q) for q in moduli]
    w = _check(pkg, oracle, moduli, top, s * DELTA, [(frac, s, top)])
    assert w.has_pre == [0] and w.scale_after == s * DELTA
    w = _check(pkg, oracle, moduli, top, s * DELTA * 8, [(frac, s, top)])
    assert w.has_pre == [0] and w.scale_after == s * DELTA * 8
    assert w.lo[0] != _check(pkg, oracle, moduli, top, s * DELTA, [(frac, s, top)]).lo[0]          # scaled by res.scale / ct.scale, not by Delta
    # --- with an integer-valued constant (:544): the receiver's scale above, equal to and below ct.scale
    w = _check(pkg, oracle, moduli, top, s * 4, [(whole, s, top)])
    assert w.has_pre == [0] and w.scale_after == s * 4
    w = _check(pkg, oracle, moduli, top, s, [(whole, s, top)])
    assert w.has_pre == [0] and w.scale_after == s
    w = _check(pkg, oracle, moduli, top, s, [(whole, s * 4, top)])
    assert w.has_pre == [1] and w.quirk == [False] and w.scale_after == s * 4 and w.pre[0] == [ref.mform(4, q) for q in moduli]
    # --- the truncating equalisation: a ratio in [1, 2) becomes the word 1, on either side
    w = _check(pkg, oracle, moduli, top, s * DELTA, [(frac, s * (1 + 2.0 ** -21), top)])
    assert w.has_pre == [1] and w.pre[0] == [ref.mform(1, q) for q in moduli] and w.scale_after == DELTA * (s * (1 + 2.0 ** -21))
    # --- the :553 quirk: a float64 ratio with a fractional part is scaled by Delta inside MultByConst, the scale is overwritten at :556
    w = _check(pkg, oracle, moduli, top, s, [(whole, s * 1.5, top)])
    assert w.has_pre == [1] and w.quirk == [True] and w.scale_after == s * 1.5
    assert w.pre[0] == [ref.mform(int(1.5 * DELTA) % q, q) for q in moduli]
    # --- real, imaginary and mixed constants, fractional and whole, positive and negative; with and without AddConst
    consts = [0.75, -0.75, 0.375j, -0.375j, 0.1 - 0.7j, 5.0, -5.0, 7j, -7j, -2 + 9j, 0j, 2.0 ** 62, -(2.0 ** 62) * 1j, 1e-300 + 0j]
    for c in consts:
        for c0 in (None, c, 0.5 + 0.5j):
            _check(pkg, oracle, moduli, top, s, [(c, s, top)], c0)
    w = _check(pkg, oracle, moduli, top, s, [(0.75, s, top)], c0=-0.75)
    assert w.add[0] == w.add[1]                                                                # a real constant: one word for both halves
    w = _check(pkg, oracle, moduli, top, s, [(0.375j, s, top)], c0=0.375j)
    assert w.add[0] != w.add[1] and w.lo[0] != w.hi[0]
    assert [(a + b) % q for a, b, q in zip(w.add[0], w.add[1], moduli)] == [0] * len(moduli)    # +-b psi^(N/2)
    # --- a negative constant whose scaled value is a multiple of q leaves q itself (scaleUpExact: res = q - 0), real and imaginary
    for i, q in enumerate(moduli):
        if q < 2 ** 53:
            w = _check(pkg, oracle, moduli, top, s, [(-float(q), s, top), (-float(q) * 1j, s, top), (-float(2 * q), s, top)], c0=-float(q) / s)
            assert w.lo[0][i] == ref.mform(q, q) == w.lo[2][i] and w.add[0][i] == q
            assert enc_ref.scale_up_exact(-float(q), 1.0, q) == q
    assert any(q < 2 ** 53 for q in moduli) or name == "qi60"
    # --- terms at three levels, the receiver above, between and below them: words for the limbs 0 .. level_after in the terms' order
    for res_level, want_level in ((top, 1), (2, 1), (0, 0)):
        w = _check(pkg, oracle, moduli, res_level, s, [(frac, s, top), (whole, s * 2, 1), (-frac, s, 2)], c0=1 - 1j)
        assert w.level_after == want_level and len(w.lo[0]) == want_level + 1
    # --- a chain that changes the receiver's scale at every step, and no term at all
    _check(pkg, oracle, moduli, top, s, [(frac, s, top), (whole, s * 3, top), (frac, s * 1.25, top), (whole, s / 8, top), (frac, s, top)], c0=0.3j)
    w = _check(pkg, oracle, moduli, 2, s * 3, [], c0=0.3j)
    assert w.level_after == 2 and w.scale_after == s * 3
    w = _check(pkg, oracle, moduli, 2, s * 3, [])
    assert w.level_after == 2 and w.add is None
    # --- a default scale of exactly 1 never takes the :522 branch (scale != 1 is what the reference asks)
    w = _check(pkg, oracle, moduli, top, 4.0, [(frac, 8.0, top)], delta=1.0)
    assert w.has_pre == [1] and w.scale_after == 8.0


def test_seeded_chains(pkg, oracle):
    """random chains: constants with and without fractional parts and zero parts, scales around Delta, its square and far from both"""
    sets = _sets(pkg)
    rng = np.random.default_rng(20240611)
    inside = 0
    for it in range(150):
        moduli = sets[("qi60", "ckks", "limit")[it % 3]]
        top = len(moduli) - 1
        pick_scale = lambda: float(2.0 ** rng.integers(30, 60) * rng.choice([1.0, 1.0, 1.5, 1 + 2.0 ** -30, rng.uniform(1, 2)]))

        def pick_const():
            part = lambda: float(rng.choice([0.0, rng.integers(-9, 10), rng.uniform(-1, 1), rng.integers(-2 ** 40, 2 ** 40), rng.uniform(-1e6, 1e6)]))
            return complex(part(), part())
        terms = [(pick_const(), pick_scale(), int(rng.integers(0, top + 1))) for _ in range(rng.integers(0, 6))]
        c0 = pick_const() if rng.integers(0, 2) else None
        res_level, res_scale = int(rng.integers(0, top + 1)), pick_scale()
        try:
            ref.constants(moduli, _psi1(oracle, moduli), DELTA, res_level, res_scale, terms, c0)
        except ref.DomainError:                                        # (a ratio of 2^63 or more: the library refuses as well)
            with pytest.raises(pkg.ring.LatticeRingError) as e:
                pkg.ring.ckks_lincomb_constants(moduli, _psi1(oracle, moduli), DELTA, res_level, res_scale, terms, c0)
            assert e.value.code == 4
            continue
        _check(pkg, oracle, moduli, res_level, res_scale, terms, c0)
        inside += 1
    assert inside >= 100


def test_a_ratio_never_truncates_to_zero():
    rng = np.random.default_rng(5)
    for _ in range(2000):
        y = float(2.0 ** rng.integers(-300, 300) * rng.uniform(1, 2))
        for x in (math.nextafter(y, math.inf), y * (1 + 2.0 ** -40), y * rng.uniform(1, 4)):
            if x > y:
                assert math.trunc(x / y) >= 1


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def _raw(pkg, moduli, psi, delta, res_level, res_scale, terms, c0, nulls=()):
    """the C call itself on sentinel-filled outputs; returns (status, message, outputs untouched?)"""
    lib = pkg._native.lib()
    T, L = len(terms), len(moduli)
    u64s = lambda v: (C.c_uint64 * max(len(v), 1))(*[int(x) for x in v])
    dbl = lambda v: (C.c_double * max(len(v), 1))(*[float(x) for x in v])
    cs = [complex(t[0]) for t in terms]
    outs = {"level_after": C.c_int(-7), "scale_after": C.c_double(-7.0), "add_lo": np.full(L, 7, dtype=np.uint64), "add_hi": np.full(L, 7, dtype=np.uint64),
            "has_pre": np.full(max(T, 1), 7, dtype=np.uint8), "pre": np.full(max(T * L, 1), 7, dtype=np.uint64),
            "lo": np.full(max(T * L, 1), 7, dtype=np.uint64), "hi": np.full(max(T * L, 1), 7, dtype=np.uint64)}
    p = lambda n: None if n in nulls else (C.byref(outs[n]) if n in ("level_after", "scale_after") else outs[n].ctypes.data_as(C.c_void_p))
    z = complex(c0) if c0 is not None else 0j
    rc = lib.lr_ckks_lincomb_constants(None if "moduli" in nulls else u64s(moduli), None if "psi" in nulls else u64s(psi), L, delta, res_level, res_scale,
                                       0 if c0 is None else 1, z.real, z.imag, T, None if "term_re" in nulls else dbl([c.real for c in cs]),
                                       dbl([c.imag for c in cs]), dbl([t[1] for t in terms]), (C.c_int * max(T, 1))(*[int(t[2]) for t in terms]),
                                       p("level_after"), p("scale_after"), p("add_lo"), p("add_hi"), p("has_pre"), p("pre"), p("lo"), p("hi"))
    untouched = outs["level_after"].value == -7 and outs["scale_after"].value == -7.0 and all((outs[n] == 7).all() for n in ("add_lo", "add_hi", "has_pre", "pre", "lo", "hi"))
    return rc, lib.lr_last_error_string().decode(), untouched


def test_domain_refusals_write_nothing(pkg, oracle):
    moduli = _sets(pkg)["ckks"]
    psi = _psi1(oracle, moduli)
    top, s = len(moduli) - 1, DELTA
    ok = [(0.5, s, top)]
    inf, nan = math.inf, math.nan
    who = "CKKS linear combination constants: "
    cases = [
        (dict(nulls=("moduli",)), "null argument"), (dict(nulls=("psi",)), "null argument"), (dict(nulls=("level_after",)), "null argument"),
        (dict(nulls=("scale_after",)), "null argument"), (dict(nulls=("add_lo",), c0=1.0), "null argument"), (dict(nulls=("term_re",)), "null argument"),
        (dict(nulls=("has_pre",)), "null argument"), (dict(nulls=("hi",)), "null argument"),
        (dict(res_level=-1), "a count or a level is out of range"), (dict(res_level=top + 1), "a count or a level is out of range"),
        (dict(terms=[(0.5, s, top + 1)]), "a count or a level is out of range"), (dict(terms=[(0.5, s, -1)]), "a count or a level is out of range"),
        (dict(moduli=[moduli[0] + 1] + moduli[1:]), "a modulus is even, below 3 or not below 2^61"),
        (dict(moduli=[1] + moduli[1:]), "a modulus is even, below 3 or not below 2^61"),
        (dict(moduli=[(1 << 61) + 1] + moduli[1:]), "a modulus is even, below 3 or not below 2^61"),
        (dict(psi=[moduli[0]] + psi[1:]), "a root word is not below its modulus"),
        (dict(delta=0.0), "a scale is not finite and positive"), (dict(delta=inf), "a scale is not finite and positive"),
        (dict(res_scale=-s), "a scale is not finite and positive"), (dict(res_scale=nan), "a scale is not finite and positive"),
        (dict(terms=[(0.5, 0.0, top)]), "a scale is not finite and positive"), (dict(terms=[(0.5, inf, top)]), "a scale is not finite and positive"),
        (dict(c0=complex(inf, 0)), "a constant is not finite and below 2^63 in magnitude"), (dict(c0=complex(0, nan)), "a constant is not finite and below 2^63 in magnitude"),
        (dict(c0=2.0 ** 63), "a constant is not finite and below 2^63 in magnitude"),
        (dict(terms=[(-(2.0 ** 63), s, top)]), "a constant is not finite and below 2^63 in magnitude"),
        (dict(terms=[(complex(0.5, -inf), s, top)]), "a constant is not finite and below 2^63 in magnitude"),
        # uint64((Delta * ct.scale) / res.scale) at :528 and uint64(ct.scale / res.scale) at :552, from 2^63 on
        (dict(terms=[(0.5, 2.0 ** 63, top)], res_scale=s), "a scale ratio is not below 2^63"),
        (dict(terms=[(3.0, s * 2.0 ** 63, top)], res_scale=s), "a scale ratio is not below 2^63"),
        (dict(terms=[(0.5, 1e300, top)], delta=1e300), "a scale ratio is not below 2^63"),                       # Delta * ct.scale = +Inf
        # a product that scaleUpExact would hand to big.NewFloat as an infinity
        (dict(c0=2.0 ** 62, res_scale=1e300), "a constant times its scale is not finite"),
        (dict(terms=[(2.0 ** 62, 1e-300, top)], res_scale=1e300), "a constant times its scale is not finite"),   # scale = res.scale / ct.scale = +Inf
        (dict(terms=[(2.0, 1.5, top)], res_scale=1.0, delta=1.5e308), "a constant times its scale is not finite"),  # the :553 ratio times Delta
    ]
    base = dict(moduli=moduli, psi=psi, delta=DELTA, res_level=top, res_scale=s, terms=ok, c0=None, nulls=())
    rc, _, _ = _raw(pkg, **base)
    assert rc == 0
    for change, message in cases:
        rc, msg, untouched = _raw(pkg, **dict(base, **change))
        assert rc == 4 and msg == who + message and untouched, (change, rc, msg, untouched)
        if not change.get("nulls") and "moduli" not in change and "psi" not in change:
            args = dict(base, **change)
            with pytest.raises(ref.DomainError):
                ref.constants(args["moduli"], args["psi"], args["delta"], args["res_level"], args["res_scale"], args["terms"], args["c0"])
    # the edge of the domain is inside it
    edge = math.nextafter(2.0 ** 63, 0)
    _check(pkg, oracle, moduli, top, s, [(complex(edge, -edge), s, top), (3.0, s * edge, top)], c0=complex(-edge, edge))


# ---- what the chain means --------------------------------------------------------------------------------------------------------
def test_the_restated_chain_computes_the_linear_combination(pkg, oracle):
    """"Ciphertexts" (pt_k, 0) with pt_k the encoder restatement's encoding of random real slot vectors v_k in [-1, 1], scales that differ
    from 2^40 by relative amounts below 2^-20, mixed levels; the restated chain, decoded at scale_after, against c0 + sum c_k v_k for four
    terms with |c_k| <= 1.  Bound: every slot within 2^-15, the precision the reference's own test demands (ckks/ckks_test.go:60,
    medianprec = 15).  The reference equalises scales by truncation (uint64(ratio) -> 1, asserted to happen here): each such step leaves a
    relative error below the scale spread on the running sum, four steps of 2^-20 on values of magnitude <= 5 stay below 2^-15.  The :553
    branch is left out (fractional constants only): there the reference itself is off by a factor Delta."""
    N, Q = 32, list(pkg.params.Qi60()[:3])
    oc = oracle.Context(N, Q)
    psi = [int(v) for v in oc.ntt_psi[:, 1]]
    enc = enc_ref.Encoder(oracle, N, Q)
    rng = np.random.default_rng(99)
    slots = N // 2
    spreads = [1 + 2.0 ** -21, 1 - 2.0 ** -22, 1 + 2.0 ** -20.5, 1.0]
    levels = [2, 1, 2, 2]
    cs = [0.6 - 0.3j, -0.45 + 0j, 0.125j + 0.7, -0.9j + 0.05]
    c0 = 0.3 - 0.4j
    assert all(abs(c) <= 1 for c in cs) and all(abs(s - 1) < 2.0 ** -20 for s in spreads)
    vs = [rng.uniform(-1, 1, slots) for _ in cs]
    scales = [DELTA * s for s in spreads]
    cts = [(enc.encode(v.astype(np.complex128), lvl, sc), np.zeros((lvl + 1, N), dtype=np.uint64)) for v, lvl, sc in zip(vs, levels, scales)]
    # res = NewCiphertext(params, 1, C[1].Level(), C[1].Scale()), polynomial_evaluation.go:144
    k = ref.constants(Q, psi, DELTA, levels[0], scales[0], list(zip(cs, scales, levels)), c0)
    assert not any(k.quirk) and k.level_after == 1
    assert any(k.has_pre[i] and k.pre[i] == [ref.mform(1, q) for q in Q[:2]] for i in range(1, 4))        # a truncating equalisation took place
    res0, res1 = ref.elements(oc, k.level_after, cts, k.has_pre, k.pre, k.lo, k.hi, add=k.add)
    assert not res1.any()
    got = enc.decode(res0, slots, k.level_after, k.scale_after)
    want = c0 + sum(c * v for c, v in zip(cs, vs))
    err = np.max(np.abs(got - want))
    print("largest slot error %.3g (bound %.3g)" % (err, 2.0 ** -15))
    assert err < 2.0 ** -15
