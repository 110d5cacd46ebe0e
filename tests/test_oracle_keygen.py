"""The restatement of the key generators (tests/keygen_ref.py) means what key generation says, with Python integers as the arbiter.

Identity.  Whatever order the reference's lines add in, every row j of every digit i of a switching key satisfies, coefficient by
coefficient in the NTT domain,

    evk[i][0] + a_i skOut R^-1 - [j in digit i] (P mod q_j) skIn  ==  NTT(e_i) R        (mod q_j),   R = 2^64,

(a_i skOut R^-1 is MRed(a_i, skOut), NTT(e_i) R is MForm(NTT(e_i)), skIn the Montgomery residues of sk^2, of PermuteNTT(sk) or of the
caller's key), and a public key satisfies pk0 + sk pk1 R^-1 + NTT(e) == 0.  Both are checked with Python integers on n16 (N = 16, two
60-bit limbs of Q, one of P), on a ragged shape whose last digit owns one row, and on |P| = 2.

Scheme agreement.  ckks/keygen.go multiplies skIn by P inside newSwitchingKey and breaks its digit loop at |Q| - 1; bfv/keygen.go
multiplies before the powers of sk and breaks at |Q| + |P| - 1.  The two restatements give the same bits on the same inputs: that is what
lets lr_keygen serve both schemes with one path.

Chain.  Encode -> Encrypt (pk) -> MulRelin -> Rescale -> Rotate -> Decrypt -> Decode at PN12QP109 on the oracle with generated keys only;
its largest slot error over seeds 0 .. 2 is keygen_ref.CHAIN_MEASURED.  CPU only."""
import numpy as np
import pytest

import ckks_encoder_ref as encoder_ref
import keygen_ref as ref

R = 1 << 64
CHAIN_SEEDS = (0, 1, 2)


def _shape(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    N, Q, P = pkg.params.ckks_moduli("PN14QP438")
    if name == "ragged":
        return 1 << 5, list(Q[:5]), list(P)          # alpha = 2, beta = 3: the last digit owns one row
    return 1 << 5, list(Q[:4]), list(P)              # "alpha2": alpha = 2, beta = 2


def _ints(a):
    return [int(v) for v in a]


def _inputs(N, Q, P, seed):
    rng = np.random.default_rng(seed)
    QP, beta = Q + P, -(-len(Q) // len(P))
    d = {"bits": (ref.draw(rng, (N >> 3,)), ref.draw(rng, (N >> 3,))), "bits2": (ref.draw(rng, (N >> 3,)), ref.draw(rng, (N >> 3,))),
         "e": ref.draw(rng, shape_noise=(2, beta, N)), "a": ref.uniform(rng, QP, N, 2 * beta).reshape(2, beta, len(QP), N),
         "pk_e": ref.draw(rng, shape_noise=(N,)), "pk1": ref.uniform(rng, QP, N)}
    d["e"][0, 0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
    d["a"][0, 0, :, 2] = 0                                                  # a zero product: q - MRed = q
    d["a"][0, 0, :, 3] = np.array(QP, dtype=np.uint64) - np.uint64(1)
    return d


def _check_identity(kg, key, skIn, skOut, e_bytes, a):
    """skIn: the Montgomery residues before the multiplication by P"""
    N, nQ = kg.N, len(kg.Q)
    for i in range(kg.beta):
        ntt_e = kg.ctx.ntt(ref.expand_gaussian(kg.moduli, e_bytes[i], N))
        for j, q in enumerate(kg.moduli):
            own = i * kg.alpha <= j < min((i + 1) * kg.alpha, nQ)
            r_inv, p = pow(R, -1, q), kg.Pbig % q
            for x, ai, so, si, en in zip(_ints(key[2 * i][j]), _ints(a[i][j]), _ints(skOut[j]), _ints(skIn[j]), _ints(ntt_e[j])):
                assert x < q, ("not a canonical residue", i, j)
                assert (x + ai * so * r_inv - (p * si if own else 0) - en * R) % q == 0, (i, j)
        assert np.array_equal(key[2 * i + 1], a[i]), ("the uniform half changed", i)


@pytest.mark.parametrize("scheme", ["ckks", "bfv"])
@pytest.mark.parametrize("name", ["n16", "ragged", "alpha2"])
def test_identities_in_python_integers(oracle, pkg, name, scheme):
    N, Q, P = _shape(pkg, name)
    kg = ref.KeyGenerator(oracle, N, Q, P, scheme)
    d = _inputs(N, Q, P, 5)
    sk, sk2 = kg.gen_secret_key(*d["bits"]), kg.gen_secret_key(*d["bits2"])
    # the secret key is the ternary poly in Montgomery form: out of the NTT domain every limb holds 0, R mod q or -R mod q
    for row, q in zip(kg.ctx.intt(sk), kg.moduli):
        assert set(_ints(row)) <= {0, R % q, (q - R) % q}
    pk0 = kg.gen_public_key(sk, d["pk_e"], d["pk1"])
    ntt_e = kg.ctx.ntt(ref.expand_gaussian(kg.moduli, d["pk_e"], N))
    for j, q in enumerate(kg.moduli):
        r_inv = pow(R, -1, q)
        for x, s, a1, en in zip(_ints(pk0[j]), _ints(sk[j]), _ints(d["pk1"][j]), _ints(ntt_e[j])):
            assert (x + s * a1 * r_inv + en) % q == 0 and 0 < x <= q, j          # Neg of 0 is q
    # GenSwitchingKey, GenRelinKey with two powers, genrotKey
    _check_identity(kg, kg.gen_switching_key(sk2, sk, d["e"][0], d["a"][0]), sk2, sk, d["e"][0], d["a"][0])
    rlk = kg.gen_relin_keys(sk, 2, d["e"], d["a"])
    power = kg.ctx.ewise("MUL_MONT", sk, sk)
    _check_identity(kg, rlk[0], power, sk, d["e"][0], d["a"][0])
    _check_identity(kg, rlk[1], kg.ctx.ewise("MUL_MONT", power, sk), sk, d["e"][1], d["a"][1])
    for gen in (5, pow(5, -1, 2 * N), 2 * N - 1, 1):
        _check_identity(kg, kg.gen_rot_key(sk, gen, d["e"][1], d["a"][1]), kg.ctx.permute_ntt(sk, gen), sk, d["e"][1], d["a"][1])


@pytest.mark.parametrize("name", ["n16", "ragged", "alpha2"])
def test_the_two_schemes_agree_bit_for_bit(oracle, pkg, name):
    N, Q, P = _shape(pkg, name)
    ckks, bfv = ref.KeyGenerator(oracle, N, Q, P, "ckks"), ref.KeyGenerator(oracle, N, Q, P, "bfv")
    d = _inputs(N, Q, P, 6)
    sk, sk2 = ckks.gen_secret_key(*d["bits"]), ckks.gen_secret_key(*d["bits2"])
    assert np.array_equal(sk, bfv.gen_secret_key(*d["bits"]))
    assert np.array_equal(ckks.gen_public_key(sk, d["pk_e"], d["pk1"]), bfv.gen_public_key(sk, d["pk_e"], d["pk1"]))
    assert np.array_equal(ckks.gen_switching_key(sk2, sk, d["e"][0], d["a"][0]), bfv.gen_switching_key(sk2, sk, d["e"][0], d["a"][0]))
    for x, y in zip(ckks.gen_relin_keys(sk, 2, d["e"], d["a"]), bfv.gen_relin_keys(sk, 2, d["e"], d["a"])):
        assert np.array_equal(x, y)
    for gen in (5, 2 * N - 1):
        assert np.array_equal(ckks.gen_rot_key(sk, gen, d["e"][0], d["a"][0]), bfv.gen_rot_key(sk, gen, d["e"][0], d["a"][0]))


def test_pow2_galois_elements(oracle, pkg):
    N, Q, P = _shape(pkg, "n16")
    gens = ref.KeyGenerator(oracle, N, Q, P).pow2_galois_elements()
    assert len(gens) == 2 * (4 - 1) + 1 and gens[-1] == 2 * N - 1
    assert gens[:2] == [5, pow(5, -1, 2 * N)] and gens[2:4] == [25 % (2 * N), pow(25, -1, 2 * N)]


def test_chain_with_generated_keys_only(oracle, pkg):
    N, Q, P = pkg.params.ckks_moduli(ref.CHAIN_PARAMS)
    roots = encoder_ref.roots_table(N)
    worst = 0.0
    for seed in CHAIN_SEEDS:
        d = ref.oracle_chain(oracle, N, list(Q), list(P), seed, roots)
        err = float(np.max(np.abs(d["slots_out"] - d["slots_want"])))
        print("chain seed %d: largest slot error %.6e" % (seed, err))
        worst = max(worst, err)
    print("chain: largest slot error over seeds %s: %.6e (CHAIN_MEASURED = %.6e)" % (CHAIN_SEEDS, worst, ref.CHAIN_MEASURED))
    assert worst <= ref.CHAIN_TOLERANCE
    assert worst >= ref.CHAIN_MEASURED / 16, "CHAIN_MEASURED no longer describes this chain"


@pytest.mark.parametrize("name", ["n16", "ragged", "alpha2"])
def test_the_device_order_gives_the_restatements_bits(oracle, pkg, name):
    """what lr_keygen's default shape computes, in its order, over the oracle's primitives: the noise expanded with the q of (0, sign 0)
    written as 0, one transform, skIn = MRed(PermuteNTT(sk), MForm(P)) on the rows of Q only, then per row MForm, the digit's Add on the
    rows min((i + 1) alpha, |Q|) bounds, and the subtraction; relinearisation keys from the running product P sk, then x sk per power"""
    N, Q, P = _shape(pkg, name)
    kg = ref.KeyGenerator(oracle, N, Q, P, "ckks")
    ctx, nQ, d = kg.ctx, len(Q), _inputs(N, Q, P, 7)
    sk = kg.gen_secret_key(*d["bits"])
    qs = np.array(kg.moduli, dtype=np.uint64)[:, None]

    def finish(skin_q, e_bytes, a):
        key = np.zeros((2 * kg.beta, len(kg.moduli), N), dtype=np.uint64)
        for i in range(kg.beta):
            x = ref.expand_gaussian(kg.moduli, e_bytes[i], N)
            x = ctx.ewise("MFORM", ctx.ntt(np.where(x == qs, np.uint64(0), x)))
            d0, d1 = i * kg.alpha, min((i + 1) * kg.alpha, nQ)
            own = np.zeros_like(x)
            own[d0:d1] = skin_q[d0:d1]
            x[d0:d1] = ctx.ewise("ADD", x, own)[d0:d1]
            key[2 * i + 1] = a[i]
            key[2 * i] = ctx.ewise("MUL_MONT_AND_SUB", a[i], sk, out=x)
        return key
    for gen in (5, 2 * N - 1, 1):
        skin = kg.mul_by_p(ctx.permute_ntt(sk, gen))[:nQ]
        assert np.array_equal(finish(skin, d["e"][0], d["a"][0]), kg.gen_rot_key(sk, gen, d["e"][0], d["a"][0])), gen
    x = kg.mul_by_p(sk)
    for i, want in enumerate(kg.gen_relin_keys(sk, 2, d["e"], d["a"])):
        x = ctx.ewise("MUL_MONT", x, sk)
        assert np.array_equal(finish(x[:nQ], d["e"][i], d["a"][i]), want), i
