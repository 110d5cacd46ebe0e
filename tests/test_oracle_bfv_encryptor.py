"""The restatement of the BFV encryptor and decryptor (tests/bfv_encryptor_ref.py) means what BFV encryption says, with Python integers as
the arbiter: with keys built as bfv/keygen.go:92-133 builds them, decrypt(encrypt(m)) - m, centred, is ONE small integer polynomial, the
same in every limb.  For the fast forms it is exactly e0 + e1 s - e u (pk) or e (sk) and at most 19 (2 N + 1) in absolute value -- u, s
ternary, |e| <= 19 = floor(6 * 3.2); for the forms through P at most N + 2 -- two flooring divisions by P, one of them multiplied by s.
A wrong key exceeds the bound.  The compact expansions are checked against the sampler formulas on every edge decision.  CPU only."""
import numpy as np
import pytest

import bfv_encryptor_ref as ref

SIZES = [1 << 4, 1 << 10]


def _rings(pkg):
    return list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])


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


def _setup(oracle, pkg, N, seed):
    Q, P = _rings(pkg)
    rng = np.random.default_rng(seed)
    enc = ref.Encryptor(oracle, N, Q, P)
    sk, pk0, pk1, s = ref.keygen(oracle, N, Q + P, rng)
    pt = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q], dtype=np.uint64)
    noise = lambda: (rng.integers(0, 20, N) | (rng.integers(0, 2, N) << 7)).astype(np.uint8)
    bits = lambda: rng.integers(0, 256, N >> 3).astype(np.uint8)
    return Q, P, rng, enc, sk, pk0, pk1, s, pt, noise, bits


def _error(oracle, enc, Q, ct, sk, pt):
    dec = ref.decrypt(enc.cQ, ct, sk)
    diff = np.array([[(int(d) - int(m)) % q for d, m in zip(drow, mrow)] for drow, mrow, q in zip(dec, pt, Q)], dtype=object)
    return _centred(diff, Q)


@pytest.mark.parametrize("N", SIZES)
def test_pk_encryption_decrypts_to_the_plaintext_plus_small_noise(oracle, pkg, N):
    Q, P, rng, enc, sk, pk0, pk1, s, pt, noise, bits = _setup(oracle, pkg, N, 100 + N)
    uc, us, e0, e1 = bits(), bits(), noise(), noise()
    fast = _error(oracle, enc, Q, enc.encrypt_pk(True, pk0, pk1, uc, us, e0, e1, pt), sk, pt)
    assert max(abs(v) for v in fast) <= 19 * (2 * N + 1)
    if N <= 1 << 6:
        # the key's own noise is not returned by keygen: recover it from pk0 = -(s a + e) with Python integers, then the identity is exact
        cQP = oracle.Context(N, Q + P)
        e_pk = _centred(np.array(cQP.intt(cQP.ewise("NEG", cQP.ewise("MUL_MONT_AND_ADD", sk, pk1, out=pk0))), dtype=object)[:len(Q)], Q)
        u = _ternary_signed(uc, us, N)
        want = [a + b - c for a, b, c in zip(_signed_noise(e0), _negacyclic(_signed_noise(e1), s), _negacyclic(e_pk, u))]
        assert fast == want
    through_p = _error(oracle, enc, Q, enc.encrypt_pk(False, pk0, pk1, uc, us, e0, e1, pt), sk, pt)
    assert max(abs(v) for v in through_p) <= N + 2


@pytest.mark.parametrize("N", SIZES)
def test_sk_encryption_decrypts_to_the_plaintext_plus_small_noise(oracle, pkg, N):
    Q, P, rng, enc, sk, pk0, pk1, s, pt, noise, bits = _setup(oracle, pkg, N, 200 + N)
    e = noise()
    crp = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q + P], dtype=np.uint64)
    fast = _error(oracle, enc, Q, enc.encrypt_sk(True, sk, crp, e, pt), sk, pt)
    assert fast == _signed_noise(e)                       # c0 + c1 s = -a s + e + m + a s
    assert max(abs(v) for v in fast) <= 19 * (2 * N + 1)
    through_p = _error(oracle, enc, Q, enc.encrypt_sk(False, sk, crp, e, pt), sk, pt)
    assert max(abs(v) for v in through_p) <= N + 2


@pytest.mark.parametrize("N", SIZES)
def test_a_wrong_key_exceeds_the_bound(oracle, pkg, N):
    Q, P, rng, enc, sk, pk0, pk1, s, pt, noise, bits = _setup(oracle, pkg, N, 300 + N)
    other = ref.keygen(oracle, N, Q + P, np.random.default_rng(999))[0]
    uc, us, e0, e1, e = bits(), bits(), noise(), noise(), noise()
    crp = np.array([rng.integers(0, q, N, dtype=np.uint64) for q in Q + P], dtype=np.uint64)
    cts = [enc.encrypt_pk(True, pk0, pk1, uc, us, e0, e1, pt), enc.encrypt_pk(False, pk0, pk1, uc, us, e0, e1, pt),
           enc.encrypt_sk(True, sk, crp, e, pt), enc.encrypt_sk(False, sk, crp, e, pt)]
    for ct in cts:
        dec = ref.decrypt(enc.cQ, ct, other)
        worst = max(min((int(d) - int(m)) % q, (int(m) - int(d)) % q) for drow, mrow, q in zip(dec, pt, Q) for d, m in zip(drow, mrow))
        assert worst > 19 * (2 * N + 1)


def test_without_p_only_the_fast_forms_work(oracle, pkg):
    Q, _ = _rings(pkg)
    enc = ref.Encryptor(oracle, 16, Q, [])
    z = np.zeros((2, 16), dtype=np.uint64)
    b2, b16 = np.zeros(2, dtype=np.uint8), np.zeros(16, dtype=np.uint8)
    with pytest.raises(ValueError, match="modulus P is empty"):
        enc.encrypt_pk(False, z, z, b2, b2, b16, b16, z)
    assert enc.encrypt_pk(True, z, z, b2, b2, b16, b16, z).shape == (2, 2, 16)


def test_ternary_expansion_on_all_four_decisions(oracle, pkg):
    Q, P = _rings(pkg)
    moduli, N = Q + P, 16
    # coefficient i: (coeff, sign) = (i & 1, (i >> 1) & 1) in the first byte; the second byte all ones
    coeff = np.array([0b10101010, 0xFF], dtype=np.uint8)
    sign = np.array([0b11001100, 0xFF], dtype=np.uint8)
    pol = ref.expand_ternary(oracle, moduli, coeff, sign, N)
    for j, q in enumerate(moduli):
        plain = [oracle.inv_mform(int(v), q) for v in pol[j]]
        assert plain[:8] == [0, 1, 0, q - 1] * 2          # (0,0) -> 0, (1,0) -> 1, (0,1) -> 0, (1,1) -> q - 1
        assert plain[8:] == [q - 1] * 8
        # index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1) into [0, MForm(1), MForm(q - 1)]
        assert int(pol[j, 1]) == oracle.mform(1, q) and int(pol[j, 3]) == oracle.mform(q - 1, q) and int(pol[j, 0]) == 0


def test_gaussian_expansion_on_the_edge_bytes(oracle, pkg):
    Q, P = _rings(pkg)
    moduli, N = Q + P, 16
    e = np.zeros(N, dtype=np.uint8)
    e[:6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
    pol = ref.expand_gaussian(moduli, e, N)
    for j, q in enumerate(moduli):
        # (coeff & sign mask) | ((q - coeff) & ~sign mask), ring/gaussianSampler.go:247: (0, sign 0) is q, not 0
        assert [int(v) for v in pol[j, :6]] == [q, 0, q - 19, 19, q - 127, 127]
        assert all(int(v) == q for v in pol[j, 6:])
    # and Context.Add takes the residue q as zero: CRed(x + q) = x
    ctx = oracle.Context(N, moduli)
    x = np.array([[5] * N for _ in moduli], dtype=np.uint64)
    assert [int(v) for v in ctx.ewise("ADD", x, pol)[0, :4]] == [5, 5, (5 - 19) % moduli[0], 24]


@pytest.mark.parametrize("degree", [0, 1, 2, 7, 8, 9])
def test_decrypt_is_horner_at_the_key(oracle, pkg, degree):
    """sum ct[i] s^i modulo every q_j, for the cadence's degrees (i & 7 == 7 inside the loop, the skipped final Reduce)"""
    Q, _ = _rings(pkg)
    N = 16
    rng = np.random.default_rng(degree)
    cQ = oracle.Context(N, Q)
    s = [int(v) for v in rng.integers(-1, 2, N)]
    sk = cQ.ntt(np.array([[oracle.mform(v % q, q) for v in s] for q in Q], dtype=np.uint64))
    ct = np.array([[rng.integers(0, q, N, dtype=np.uint64) for q in Q] for _ in range(degree + 1)], dtype=np.uint64)
    got = ref.decrypt(cQ, ct, sk)
    for j, q in enumerate(Q):
        acc = [int(v) for v in ct[degree, j]]
        for i in range(degree, 0, -1):
            acc = [(a + int(c)) % q for a, c in zip(_negacyclic(acc, s), ct[i - 1, j])]
        assert [int(v) for v in got[j]] == [a % q for a in acc]
