"""The restatement of collective key switching (tests/collective_ref.py) means what the protocols say, with Python integers as the arbiter.

Identities.  A CKS share is the division by P of X = P c1 (s_in - s_out) + e, an integer polynomial over Q_level P that Python computes
from the keys and the signed decisions; a PCKS share is the division by P of X_k = u pk_k + e_k, plus s c1 on component 0.  The ModDowns
compute (X - [X]_P) / P with [X]_P from modUpExact (ring_basis_extension.go:352-393), whose float correction index v can be off by one
when the float64 sum rounds across an integer: the result is within 1 per coefficient of round(X / P), the same small difference in every
limb -- the bound and the reasoning of tests/test_oracle_ckks_encryptor.py.  Every residue is canonical.  Shapes: n16 (N = 16, two 60-bit
limbs of Q, one of P), |P| = 2 (N = 32, the first 4 Q and both P of CKKS PN14QP438) and BFV's PN13QP218 moduli at N = 32; CKKS shares at
the top level and at level 0.  The inputs carry the edge decisions: noise bytes (0, +) (0, -) (19, +-) (127, +-), sk_in == sk_out on one
NTT coefficient (Delta = CRed(q) = 0), c1 coefficients 0 and q_j - 1.

Protocols.  Three parties with additive secret shares, a ciphertext under the collective public key keygen_ref makes from the summed
secret, three shares with sigma = 6.36 bytes, the fold, KeySwitch, Decrypt under the summed output secret (CKS) or the target secret
(PCKS): BFV at PN12QP109 with t = 65537 decodes to the plaintext exactly; CKKS at PN12QP109, scale 2^30, top level and level 0, decodes
within collective_ref.SWITCH_TOLERANCE = 16 x the largest slot error measured here over seeds 0 .. 2.

The fold in the device's order (32 shares per pass, the running sum the first term of the next) is n - 1 Context.Add calls.  The device's
default shapes, restated in their order over the oracle's primitives, give the restatement's bits; for BFV CKS that includes writing 0
where the reference leaves p_j in hP.  CPU only."""
import numpy as np
import pytest

import collective_ref as ref
import keygen_ref

SEEDS = (0, 1, 2)


def _shape(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    if name == "alpha2":
        _, Q, P = pkg.params.ckks_moduli("PN14QP438")
        return 1 << 5, list(Q[:4]), list(P)
    _, Q, P, _ = pkg.params.bfv_moduli("PN13QP218")
    return 1 << 5, list(Q), list(P)


SHAPES = ["n16", "alpha2", "bfv"]


def _prod(moduli):
    out = 1
    for m in moduli:
        out *= int(m)
    return out


def _crt(rows, moduli):
    """[limbs, N] residues -> the integers in [0, prod moduli)"""
    M = _prod(moduli)
    hats = [M // q for q in moduli]
    invs = [pow(h % q, -1, q) for h, q in zip(hats, moduli)]
    return [sum(int(rows[j][i]) * invs[j] % q * hats[j] for j, q in enumerate(moduli)) % M for i in range(len(rows[0]))]


def _negacyclic(a, b, M):
    """a * b in Z_M[X] / (X^N + 1) with Python integers"""
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
    return [v % M for v in out]


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


def _plain_coeffs(oracle, N, moduli, rows_ntt_mont):
    """a key's rows (NTT + Montgomery form over `moduli`) -> its integer coefficients modulo prod moduli"""
    ctx = oracle.Context(N, moduli)
    return _crt(ctx.intt(ctx.ewise("INV_MFORM", np.ascontiguousarray(rows_ntt_mont))), moduli)


def _inputs(oracle, N, Q, P, seed):
    rng = np.random.default_rng(seed)
    QP, nQ = Q + P, len(Q)
    kg = keygen_ref.KeyGenerator(oracle, N, Q, P)
    bits = lambda: (keygen_ref.draw(rng, (N >> 3,)), keygen_ref.draw(rng, (N >> 3,)))
    d = {"sk_in": kg.gen_secret_key(*bits()), "sk_out": kg.gen_secret_key(*bits()), "u": bits()}
    d["sk_out"][:, 3] = d["sk_in"][:, 3]                                   # Delta = CRed((x + q) - x) = CRed(q) = 0 there
    d["pk1"] = keygen_ref.uniform(rng, QP, N)
    d["pk0"] = kg.gen_public_key(kg.gen_secret_key(*bits()), keygen_ref.draw(rng, shape_noise=(N,)), d["pk1"])
    c1 = keygen_ref.uniform(rng, Q, N)
    c1[:, 1] = 0
    c1[:, 2] = np.array(Q, dtype=np.uint64) - np.uint64(1)
    d["c1"] = c1
    d["e"] = [ref.edge_bytes(ref.smudging_bytes(rng, N)) for _ in range(3)]
    d["e"][1] = np.roll(d["e"][1], 5)
    return d


def _assert_divided(oracle, N, Ql, P, coeff_rows, X, plus, what):
    """coeff_rows [level + 1, N], coefficient domain: canonical residues of round(X / P) + plus modulo Q_level, within 1 per coefficient"""
    Pint, Mq = _prod(P), _prod(Ql)
    for row, q in zip(coeff_rows, Ql):
        assert all(int(v) < q for v in row), (what, "not a canonical residue")
    got = _crt(coeff_rows, Ql)
    for g, x, a in zip(got, X, plus):
        diff = (g - _round_div(x, Pint) - a) % Mq
        assert min(diff, Mq - diff) <= 1, what


@pytest.mark.parametrize("name", SHAPES)
def test_cks_shares_are_the_division_by_p(oracle, pkg, name):
    N, Q, P = _shape(pkg, name)
    col, d = ref.Collective(oracle, N, Q, P), _inputs(oracle, N, Q, P, 11)
    nQ, Pint = len(Q), _prod(P)
    zero = [0] * N
    for level in sorted({nQ - 1, 0}):
        Ql = Q[:level + 1]
        M = _prod(Ql) * Pint
        delta = _plain_coeffs(oracle, N, Ql, col.cQ.ewise("SUB", d["sk_in"][:nQ], d["sk_out"][:nQ])[:level + 1])
        e = _signed_noise(d["e"][0])
        # CKKS: c1 in the NTT domain
        cl = oracle.Context(N, Ql)
        c1 = _crt(cl.intt(d["c1"][:level + 1]), Ql)
        X = [(Pint * v + n) % M for v, n in zip(_negacyclic(c1, delta, _prod(Ql)), e)]
        share = col.ckks_cks_share(level, d["sk_in"], d["sk_out"], d["c1"], d["e"][0])
        assert share.shape == (level + 1, N)
        _assert_divided(oracle, N, Ql, P, cl.intt(share), X, zero, (name, "ckks", level))
        if level == nQ - 1:   # BFV: c1 in the coefficient domain, all of Q
            c1 = _crt(d["c1"], Q)
            X = [(Pint * v + n) % M for v, n in zip(_negacyclic(c1, delta, _prod(Q)), e)]
            _assert_divided(oracle, N, Q, P, col.bfv_cks_share(d["sk_in"], d["sk_out"], d["c1"], d["e"][0]), X, zero, (name, "bfv"))


@pytest.mark.parametrize("name", SHAPES)
def test_pcks_shares_are_the_division_by_p_plus_s_c1(oracle, pkg, name):
    N, Q, P = _shape(pkg, name)
    col, d = ref.Collective(oracle, N, Q, P), _inputs(oracle, N, Q, P, 12)
    nQ = len(Q)
    u, e = _ternary_signed(d["u"][0], d["u"][1], N), [_signed_noise(d["e"][1]), _signed_noise(d["e"][2])]
    zero = [0] * N
    for level in sorted({nQ - 1, 0}):
        Ql = Q[:level + 1]
        rows = list(range(level + 1)) + list(range(nQ, nQ + len(P)))
        M, Mq = _prod(Ql + P), _prod(Ql)
        # MRed(MForm(u), pk) = u pk: the key as it stands, out of the NTT domain, over the rows the ModDown reads
        keys = [_crt(oracle.Context(N, Ql + P).intt(np.ascontiguousarray(pk[rows])), Ql + P) for pk in (d["pk0"], d["pk1"])]
        X = [[(a + b) % M for a, b in zip(_negacyclic(u, key, M), ek)] for key, ek in zip(keys, e)]
        s = _plain_coeffs(oracle, N, Ql, d["sk_in"][:level + 1])
        cl = oracle.Context(N, Ql)
        sc1 = _negacyclic(s, _crt(cl.intt(d["c1"][:level + 1]), Ql), Mq)
        out = col.ckks_pcks_share(level, d["sk_in"], d["pk0"], d["pk1"], d["c1"], d["u"][0], d["u"][1], d["e"][1], d["e"][2])
        assert out.shape == (2, level + 1, N)
        _assert_divided(oracle, N, Ql, P, cl.intt(out[0]), X[0], sc1, (name, "ckks", level, 0))
        _assert_divided(oracle, N, Ql, P, cl.intt(out[1]), X[1], zero, (name, "ckks", level, 1))
        if level == nQ - 1:
            sc1 = _negacyclic(s, _crt(d["c1"], Q), Mq)
            out = col.bfv_pcks_share(d["sk_in"], d["pk0"], d["pk1"], d["c1"], d["u"][0], d["u"][1], d["e"][1], d["e"][2])
            _assert_divided(oracle, N, Q, P, out[0], X[0], sc1, (name, "bfv", 0))
            _assert_divided(oracle, N, Q, P, out[1], X[1], zero, (name, "bfv", 1))


def _device_fold(Q, shares, base, per_pass=32):
    """lr_collective_aggregate's default shape: per_pass shares per launch, the running sum the first term of the next launch, the base on
    the last; every addition CRed(a + b) as the kernel does it, on Python integers"""
    qs = np.array(Q, dtype=object)[:shares[0].shape[0], None]
    cred = lambda x: np.where(x >= qs, x - qs, x)
    todo, acc = [s.astype(object) for s in shares], None
    while todo:
        terms = ([acc] if acc is not None else []) + todo[:per_pass - (acc is not None)]
        todo = todo[per_pass - (acc is not None):]
        acc = terms[0]
        for t in terms[1:]:
            acc = cred(acc + t)
    if base is not None:
        acc = cred(base.astype(object) + acc)
    return acc.astype(np.uint64)


@pytest.mark.parametrize("with_base", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 33])
def test_the_fold_is_n_minus_one_adds(oracle, pkg, n, with_base):
    N, Q, P = _shape(pkg, "n16")
    col = ref.Collective(oracle, N, Q, P)
    rng = np.random.default_rng(n)
    shares = [keygen_ref.uniform(rng, Q, N) for _ in range(n)]
    shares[0][:, 0] = np.array(Q, dtype=np.uint64)                       # the residue q_j itself, first and later in the order
    shares[-1][:, 1] = np.array(Q, dtype=np.uint64)
    base = keygen_ref.uniform(rng, Q, N) if with_base else None
    want = shares[0].copy()
    for s in shares[1:]:
        want = col.cQ.ewise("ADD", want, s)
    if with_base:
        want = col.cQ.ewise("ADD", base, want)
    assert np.array_equal(col.aggregate(shares, base), want)
    assert np.array_equal(_device_fold(Q, shares, base), want)
    for level in (0,):
        assert np.array_equal(col.aggregate([s[:level + 1] for s in shares], base), want[:level + 1])


def _zero_form(moduli, e_bytes, N):
    """the noise as the device's expansion writes it: the q of (0, sign 0) as 0"""
    x = ref.expand_gaussian(moduli, e_bytes, N)
    return np.where(x == np.array(moduli, dtype=np.uint64)[:, None], np.uint64(0), x)


@pytest.mark.parametrize("name", SHAPES)
def test_the_device_order_gives_the_restatements_bits(oracle, pkg, name):
    """lr_collective's default shapes, in their order, over the oracle's primitives, on the edge decisions"""
    N, Q, P = _shape(pkg, name)
    col, d = ref.Collective(oracle, N, Q, P), _inputs(oracle, N, Q, P, 13)
    cQ, cP, nQ, bext = col.cQ, col.cP, len(Q), col.baseconverter
    pmont = [col.oracle.mform(col.Pbig % q, q) for q in Q]
    for e_bytes in d["e"]:
        assert {0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80} <= set(int(b) for b in e_bytes)

    def fused(c1_ntt, level, addend):
        delta = cQ.ewise("SUB", d["sk_in"][:nQ], d["sk_out"][:nQ])[:level + 1]
        assert all(int(v) == 0 for v in delta[:, 3])
        x = cQ.ewise("MUL_MONT", cQ.ewise("MUL_MONT", c1_ntt[:level + 1], delta), np.repeat(np.array(pmont[:level + 1], dtype=np.uint64)[:, None], N, 1))
        return x if addend is None else cQ.ewise("ADD", x, addend)
    for level in sorted({nQ - 1, 0}):
        # CKKS CKS: only the rows of Q are transformed; hP = the zero-form noise in the coefficient domain
        z = _zero_form(col.moduli, d["e"][0], N)
        share = fused(d["c1"], level, cQ.ntt(z[:level + 1]))
        got = bext.moddown_split_pq(level, cQ.intt(share), z[nQ:])       # ModDownSplitedNTTPQ on coefficient-domain operands ...
        got = cQ.ntt(got)                                                # ... and back: the division is the same integer polynomial
        want = col.ckks_cks_share(level, d["sk_in"], d["sk_out"], d["c1"], d["e"][0])
        assert np.array_equal(bext.moddown_split_ntt_pq(level, share, cP.ntt(z[nQ:])), want), (name, level)
        assert np.array_equal(got, want), (name, level, "coefficient-domain form")
        # CKKS PCKS: everything in front of the ModDowns on limbs 0 .. level and the rows of P only
        rows = list(range(level + 1)) + list(range(nQ, nQ + len(P)))
        sub = oracle.Context(N, [col.moduli[r] for r in rows])
        u = sub.ntt(np.ascontiguousarray(ref.expand_ternary(oracle, col.moduli, d["u"][0], d["u"][1], N)[rows]))
        outs = []
        for pk, eb in ((d["pk0"], d["e"][1]), (d["pk1"], d["e"][2])):
            x = sub.ewise("ADD", sub.ewise("MUL_MONT", u, np.ascontiguousarray(pk[rows])), sub.ntt(np.ascontiguousarray(_zero_form(col.moduli, eb, N)[rows])))
            outs.append(bext.moddown_split_ntt_pq(level, x[:level + 1], x[level + 1:]))
        outs[0] = cQ.ewise("MUL_MONT_AND_ADD", d["c1"][:level + 1], d["sk_in"][:level + 1], out=outs[0])
        want = col.ckks_pcks_share(level, d["sk_in"], d["pk0"], d["pk1"], d["c1"], d["u"][0], d["u"][1], d["e"][1], d["e"][2])
        assert np.array_equal(np.stack(outs), want), (name, level, "pcks")
    # BFV CKS: the residue on the rows of P with p_j written as 0 changes no bit of the ModDown's output
    e = d["e"][0].copy()
    assert 0 in set(int(b) for b in e)                                   # (0, sign 0): the reference's hP holds p_j there
    literal = col.bfv_cks_share(d["sk_in"], d["sk_out"], d["c1"], e)
    assert np.array_equal(col.bfv_cks_share(d["sk_in"], d["sk_out"], d["c1"], e, hp_zero=True), literal)
    x = cQ.ewise("ADD", cQ.intt(fused(cQ.ntt(d["c1"]), nQ - 1, None)), ref.expand_gaussian(Q, e, N))
    assert np.array_equal(bext.moddown_split_pq(nQ - 1, x, _zero_form(col.moduli, e, N)[nQ:]), literal)


def test_the_p_j_in_hP_is_taken_as_zero(oracle, pkg):
    """hP all p_j (every decision (0, sign 0)) against hP all 0, on every shape: ModDownSplitedPQ gives the same bits"""
    for name in SHAPES:
        N, Q, P = _shape(pkg, name)
        col = ref.Collective(oracle, N, Q, P)
        rng = np.random.default_rng(3)
        x = keygen_ref.uniform(rng, Q, N)
        hp = np.repeat(np.array(P, dtype=np.uint64)[:, None], N, 1)
        assert np.array_equal(col.baseconverter.moddown_split_pq(len(Q) - 1, x, hp), col.baseconverter.moddown_split_pq(len(Q) - 1, x, np.zeros_like(hp)))


@pytest.mark.parametrize("protocol", ["cks", "pcks"])
def test_bfv_switch_decodes_to_the_plaintext(oracle, pkg, protocol):
    N, Q, P, _ = pkg.params.bfv_moduli(ref.SWITCH_PARAMS)
    d = ref.oracle_switch(oracle, "bfv", protocol, N, list(Q), list(P), 0)
    assert np.array_equal(d["decoded"], d["ints"])
    # and not under the input secret
    import bfv_encoder_ref
    import bfv_encryptor_ref
    cQ = oracle.Context(N, [int(q) for q in Q])
    wrong = bfv_encoder_ref.Encoder(oracle, N, Q, ref.BFV_T).decode_uint(bfv_encryptor_ref.decrypt(cQ, d["out"], d["sk"]))
    assert not np.array_equal(wrong, d["ints"])


def test_ckks_switch_returns_the_slot_values(oracle, pkg):
    """measured maximum slot error over seeds 0 .. 2 x (cks, pcks) x (top level, level 0): SWITCH_MEASURED; allowed 16 x that"""
    import ckks_encoder_ref
    N, Q, P = pkg.params.ckks_moduli(ref.SWITCH_PARAMS)
    roots = ckks_encoder_ref.roots_table(N)
    worst = 0.0
    for seed in SEEDS:
        for protocol in ("cks", "pcks"):
            for level in (len(Q) - 1, 0):
                d = ref.oracle_switch(oracle, "ckks", protocol, N, list(Q), list(P), seed, level, roots)
                err = float(np.max(np.abs(d["decoded"] - d["values"])))
                print("switch %s seed %d level %d: largest slot error %.6e" % (protocol, seed, level, err))
                worst = max(worst, err)
    print("switch: largest slot error %.6e (SWITCH_MEASURED = %.6e)" % (worst, ref.SWITCH_MEASURED))
    assert worst <= ref.SWITCH_TOLERANCE
    assert worst >= ref.SWITCH_MEASURED / 16, "SWITCH_MEASURED no longer describes this chain"
