"""The restatement of the CKKS encryptor (tests/ckks_encryptor_ref.py) means what CKKS encryption says, with Python integers as the
arbiter, at N = 16 over two 60-bit limbs of Q and one of P, keys built as ckks/keygen.go builds them (the lines of bfv/keygen.go:92-133).

Fast forms: ct0 + ct1 s - pt, taken out of the NTT domain and centred, is ONE integer polynomial, the same in every limb, and exactly
e0 + e1 s - e_pk u (pk) or e (sk).

Forms through P: every component is the division by P of an integer polynomial X over Q||P that Python computes from the signed
decisions -- X_k = u pk_k + e_k (pk), X_0 = -crp s + e and X_1 = crp (sk).  ModDownPQ / ModDownNTTPQ compute (X - [X]_P) / P with [X]_P
from modUpExact (ring_basis_extension.go:352-393), whose correction index v is the truncation of a float64 sum of the y_i / q_i (:370,
:375).  That sum's fractional part is (X mod P) / P, so the result is floor(X / P), and the one way it can differ is v off by one when
the float64 sum rounds across an integer: floor - 1 when the fraction is just above 0, floor + 1 when it is just below 1.  Against the
rounded division round(X / P) this is a difference of at most 1 per coefficient in both cases, and that is the bound asserted here.
The decryption noise of those forms follows: (X_0 + X_1 s) / P is below 1 in absolute value, each component is within 1.5 of X_k / P,
s is ternary, so |ct0 + ct1 s - pt| <= 1.5 (N + 1) + 1.

The round trip Encode -> Encrypt -> Decrypt -> Decode runs on the restatements alone.  CPU only."""
import numpy as np
import pytest

import ckks_encoder_ref as encoder_ref
import ckks_encryptor_ref as ref

N16 = 1 << 4
FORMS = [("pk", True), ("pk", False), ("sk", True), ("sk", False)]

ROUND_TRIP_SEEDS = (0, 1, 2)
ROUND_TRIP_MEASURED, ROUND_TRIP_TOLERANCE = ref.ROUND_TRIP_MEASURED, ref.ROUND_TRIP_TOLERANCE


def _rings(pkg):
    return list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])


def _prod(moduli):
    out = 1
    for m in moduli:
        out *= m
    return out


def _crt(rows, moduli):
    """[limbs, N] residues -> the integers in [0, prod moduli)"""
    M = _prod(moduli)
    hats = [M // q for q in moduli]
    invs = [pow(h % q, -1, q) for h, q in zip(hats, moduli)]
    return [sum(int(rows[j][i]) * invs[j] % q * hats[j] for j, q in enumerate(moduli)) % M for i in range(len(rows[0]))]


def _centred(limbs, moduli):
    """[limbs, N] residues -> the integer polynomial they all agree on, centred; fails where two limbs disagree"""
    rows = []
    for row, q in zip(limbs, moduli):
        rows.append([int(v) - q if int(v) > q // 2 else int(v) for v in (int(x) % q for x in row)])
    for r in rows[1:]:
        assert r == rows[0], "the limbs disagree: not one small integer polynomial"
    return rows[0]


def _negacyclic(a, b):
    """a * b in Z[X] / (X^N + 1) with Python integers"""
    N = len(a)
    out = [0] * N
    for i, x in enumerate(a):
        if x == 0:
            continue
        for j, y in enumerate(b):
            k = i + j
            if k < N:
                out[k] += x * y
            else:
                out[k - N] -= x * y
    return out


def _signed_noise(e_bytes):
    return [(int(b) & 127) if int(b) >> 7 else -(int(b) & 127) for b in e_bytes]


def _ternary_signed(coeff_bits, sign_bits, N):
    out = []
    for i in range(N):
        c, s = (int(coeff_bits[i >> 3]) >> (i & 7)) & 1, (int(sign_bits[i >> 3]) >> (i & 7)) & 1
        out.append(0 if not c else (-1 if s else 1))
    return out


def _round_div(x, p):
    return (2 * x + p) // (2 * p)


def _setup(oracle, pkg, seed, N=N16):
    Q, P = _rings(pkg)
    rng = np.random.default_rng(seed)
    enc = ref.Encryptor(oracle, N, Q, P)
    sk, pk0, pk1, s = ref.keygen(oracle, N, Q + P, rng)
    pt = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q], dtype=np.uint64)
    noise = lambda: (rng.integers(0, 20, N) | (rng.integers(0, 2, N) << 7)).astype(np.uint8)
    bits = lambda: rng.integers(0, 256, N >> 3).astype(np.uint8)
    crp = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q + P], dtype=np.uint64)
    return Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, crp


def _noise_of(enc, level, ct, sk, pt):
    """ct0 + ct1 s - pt over limbs 0 .. level, out of the NTT domain, centred"""
    cQ, L1 = enc.cQ, level + 1
    acc = cQ.ewise("ADD", ct[0], cQ.ewise("MUL_MONT", ct[1], np.asarray(sk)[:L1]))
    acc = cQ.ewise("SUB", acc, np.asarray(pt)[:L1])
    return _centred(np.array(cQ.intt(acc, level), dtype=object), enc.Q[:L1])


def _key_noise(oracle, Q, P, sk, pk0, pk1):
    """the key's own noise, which keygen does not return: pk0 = -(s a + e)"""
    cQP = oracle.Context(N16, Q + P)
    return _centred(np.array(cQP.intt(cQP.ewise("NEG", cQP.ewise("MUL_MONT_AND_ADD", sk, pk1, out=pk0))), dtype=object), Q + P)


@pytest.mark.parametrize("level", [1, 0])
def test_pk_fast_is_exactly_the_noise_expression(oracle, pkg, level):
    Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, _ = _setup(oracle, pkg, 100 + level)
    uc, us, e0, e1 = bits(), bits(), noise(), noise()
    e0[:3], e1[:3] = [0, 0x80, 19], [127 | 0x80, 0, 127]          # (0, sign 0): the residue q goes through the transform
    ct = enc.encrypt_pk(True, level, pk0, pk1, uc, us, e0, e1, pt)
    assert ct.shape == (2, level + 1, N16)
    u, e_pk = _ternary_signed(uc, us, N16), _key_noise(oracle, Q, P, sk, pk0, pk1)
    want = [a + b - c for a, b, c in zip(_signed_noise(e0), _negacyclic(_signed_noise(e1), s), _negacyclic(e_pk, u))]
    assert _noise_of(enc, level, ct, sk, pt) == want


@pytest.mark.parametrize("level", [1, 0])
def test_sk_fast_is_exactly_the_noise_and_the_uniform_poly(oracle, pkg, level):
    Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, crp = _setup(oracle, pkg, 200 + level)
    e = noise()
    e[:3] = [0, 0x80, 127]
    crp[:, 5] = 0                                                  # a zero product: Neg gives q
    before = crp.copy()
    ct = enc.encrypt_sk(True, level, sk, crp, e, pt)
    assert np.array_equal(crp, before)
    assert np.array_equal(ct[1], crp[:level + 1])
    assert _noise_of(enc, level, ct, sk, pt) == _signed_noise(e)   # c0 + c1 s = -a s + e + m + a s


def _assert_divided_by_p(enc, comp_ntt, X, Q, P, what):
    """comp_ntt [|Q|, N] in the NTT domain is round(X / P) modulo Q within 1 per coefficient, the same small difference in every limb"""
    Pint = _prod(P)
    coeffs = enc.cQ.intt(comp_ntt)
    want = [_round_div(x, Pint) for x in X]
    diff = np.array([[(int(c) - w) % q for c, w in zip(row, want)] for row, q in zip(coeffs, Q)], dtype=object)
    assert max(abs(d) for d in _centred(diff, Q)) <= 1, what


def test_pk_through_p_is_the_division_by_p(oracle, pkg):
    Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, _ = _setup(oracle, pkg, 300)
    QP, level = Q + P, len(Q) - 1
    M = _prod(QP)
    uc, us, e0, e1 = bits(), bits(), noise(), noise()
    e0[:3], e1[:3] = [0, 0x80, 19], [127 | 0x80, 0, 127]
    ct = enc.encrypt_pk(False, level, pk0, pk1, uc, us, e0, e1, pt)
    u = _ternary_signed(uc, us, N16)
    cQP = oracle.Context(N16, QP)
    for k, (pk, e) in enumerate(((pk0, e0), (pk1, e1))):
        key = _crt(cQP.intt(pk), QP)                               # MRed(MForm(u), pk) = u pk: the key as it stands, out of the NTT domain
        X = [(a + b) % M for a, b in zip(_negacyclic(u, key), _signed_noise(e))]
        comp = ct[k] if k else enc.cQ.ewise("SUB", ct[0], pt)
        _assert_divided_by_p(enc, comp, X, Q, P, k)
    assert max(abs(v) for v in _noise_of(enc, level, ct, sk, pt)) <= 1.5 * (N16 + 1) + 1
    # and the entry point that takes the expanded polys computes the same bits from the same decisions
    up, e0p, e1p = ref.expand_pk_operands(oracle, enc, uc, us, e0, e1)
    plan = oracle.CkksPlan(enc.cQ, oracle.Context(N16, P))
    assert np.array_equal(plan.encrypt_pk(cQP, level, up, pk0, pk1, e0p, e1p, pt), ct)


def test_sk_through_p_is_the_division_by_p(oracle, pkg):
    Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, crp = _setup(oracle, pkg, 400)
    QP, level = Q + P, len(Q) - 1
    M = _prod(QP)
    e = noise()
    e[:3] = [0, 0x80, 127]
    crp[:, 5] = 0
    before = crp.copy()
    ct = enc.encrypt_sk(False, level, sk, crp, e, pt)
    assert np.array_equal(crp, before)
    cQP = oracle.Context(N16, QP)
    a = _crt(cQP.intt(crp), QP)
    X0 = [(b - c) % M for b, c in zip(_signed_noise(e), _negacyclic(a, s))]
    _assert_divided_by_p(enc, enc.cQ.ewise("SUB", ct[0], pt), X0, Q, P, 0)
    _assert_divided_by_p(enc, ct[1], a, Q, P, 1)
    assert max(abs(v) for v in _noise_of(enc, level, ct, sk, pt)) <= 1.5 * (N16 + 1) + 1


def test_a_wrong_key_exceeds_the_bound(oracle, pkg):
    Q, P, enc, sk, pk0, pk1, s, pt, noise, bits, crp = _setup(oracle, pkg, 500)
    level = len(Q) - 1
    other = ref.keygen(oracle, N16, Q + P, np.random.default_rng(999))[0]
    cts = [enc.encrypt_pk(True, level, pk0, pk1, bits(), bits(), noise(), noise(), pt), enc.encrypt_sk(False, level, sk, crp, noise(), pt)]
    for ct in cts:
        acc = enc.cQ.intt(enc.cQ.ewise("SUB", enc.cQ.ewise("ADD", ct[0], enc.cQ.ewise("MUL_MONT", ct[1], other[:len(Q)])), pt))
        worst = max(min(int(d) % q, -int(d) % q) for row, q in zip(acc, Q) for d in row)
        assert worst > 19 * (2 * N16 + 1)


def test_without_p_only_the_fast_forms_work(oracle, pkg):
    Q, _ = _rings(pkg)
    enc = ref.Encryptor(oracle, 16, Q, [])
    z = np.zeros((2, 16), dtype=np.uint64)
    b2, b16 = np.zeros(2, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    with pytest.raises(ValueError, match="modulus P is empty"):
        enc.encrypt_pk(False, 1, z, z, b2, b2, b16, b16, z)
    with pytest.raises(ValueError, match="modulus P is empty"):
        enc.encrypt_sk(False, 1, z, z, b16, z)
    assert enc.encrypt_pk(True, 1, z, z, b2, b2, b16, b16, z).shape == (2, 2, 16)


def test_the_transform_takes_the_residue_q_as_zero(oracle, pkg):
    """SampleNTT transforms a poly that holds q where the sampler decided (0, sign 0): Context.NTT ends on a full reduction, so the result
    is the transform of the same poly with 0 there -- what the device's expansion writes"""
    Q, _ = _rings(pkg)
    cQ = oracle.Context(N16, Q)
    e = (np.arange(N16) % 7).astype(np.uint8)                     # sign 0 everywhere, zeros at 0, 7, 14
    pol = ref.expand_gaussian(Q, e, N16)
    assert all(int(pol[j, 0]) == q for j, q in enumerate(Q))
    canon = np.array([[int(v) % q for v in pol[j]] for j, q in enumerate(Q)], dtype=np.uint64)
    assert np.array_equal(cQ.ntt(pol), cQ.ntt(canon))


def _round_trip_errors(oracle, pkg):
    N, Q, P = pkg.params.ckks_moduli("PN12QP109")
    Q, P = list(Q), list(P)
    level, scale, slots = len(Q) - 1, 2.0 ** 32, N >> 1
    enc, coder = ref.Encryptor(oracle, N, Q, P), encoder_ref.Encoder(oracle, N, Q)
    worst = 0.0
    for seed in ROUND_TRIP_SEEDS:
        rng = np.random.default_rng(7000 + seed)
        sk, pk0, pk1, _ = ref.keygen(oracle, N, Q + P, rng)
        vals = rng.uniform(0, 1, slots) * np.exp(2j * np.pi * rng.uniform(0, 1, slots))
        pt = coder.encode(vals, level, scale)
        noise = lambda: (rng.integers(0, 20, N) | (rng.integers(0, 2, N) << 7)).astype(np.uint8)
        bits = lambda: rng.integers(0, 256, N >> 3).astype(np.uint8)
        for form, fast in FORMS:
            if form == "pk":
                ct = enc.encrypt_pk(fast, level, pk0, pk1, bits(), bits(), noise(), noise(), pt)
            else:
                crp = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q + P], dtype=np.uint64)
                ct = enc.encrypt_sk(fast, level, sk, crp, noise(), pt)
            got = coder.decode(ref.decrypt(oracle, enc, level, ct, sk), slots, level, scale)
            worst = max(worst, float(np.max(np.abs(got - vals))))
    return worst


def test_round_trip_returns_the_slot_values(oracle, pkg):
    """Encode (tests/ckks_encoder_ref.py) -> Encrypt -> Decrypt -> Decode on the restatements at PN12QP109, every form, seeds 0 .. 2:
    measured maximum slot error ROUND_TRIP_MEASURED = 5.192493e-05, allowed 16 x that = ROUND_TRIP_TOLERANCE = 8.307989e-04"""
    worst = _round_trip_errors(oracle, pkg)
    print("round trip: largest slot error %.6e (recorded %.6e, allowed %.6e)" % (worst, ROUND_TRIP_MEASURED, ROUND_TRIP_TOLERANCE))
    assert worst <= ROUND_TRIP_TOLERANCE
