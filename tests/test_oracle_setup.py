"""The restatement of the collective key setup (tests/setup_ref.py) means what the protocols say, with Python integers as the arbiter, for
three parties on n16 (N = 16, two 60-bit limbs of Q, one of P), on a ragged shape whose last digit owns one row, and on |P| = 2.

Identities, with s = sum s_i, every quantity taken out of Montgomery form, w_i the CRT idempotent of digit i (1 on its rows, 0 elsewhere):

    CKG     pk0 + s crs                          ==  sum e_i                                  exactly
    RKG     key[i][0] + s key[i][1] - P s^2 w_i  ==  s E1 + E2 + u E3 + E4                    small
    naive   key[i][0] + s key[i][1] - P s^2 w_i  ==  s E0 U + s F0 + E0 V + G0 + s^2 F1 + s G1  small
    RTG     key[i][0] + s key[i][1] - P pi(s) w_i ==  sum e_i                                 exactly

(capitals are sums over the parties: E* the noise of the rounds, U and V the naive rounds' ternaries, E0 the CKG noise inside pk0).
"Small" is the worst-case sum of those terms: a ternary sum is at most n in absolute value, a noise sum at most 127 n, and a product of
two polys of the negacyclic ring grows by at most the weight h of the ternary factor (h = N: a bit plane may be all ones):

    RKG     2 h n (127 n) + 2 (127 n)
    naive   127 n (2 h^2 n^2 + 3 h n + 1)

Further: the two schemes' lines agree bit for bit wherever they coincide; dckks/relinkey_gen_naive.go:73-75 is pinned; the device's fused
order gives the restatement's bits; the RTG share equals lr_keygen's evakey[i][0] once the uniform half is MForm(crp).  CPU only."""
import numpy as np
import pytest

import keygen_ref
import setup_ref as ref

R = 1 << 64
N_PARTIES = ref.PARTIES
MAG = 127


def _shape(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    N, Q, P = pkg.params.ckks_moduli("PN14QP438")
    if name == "ragged":
        return 1 << 5, list(Q[:5]), list(P)          # alpha = 2, beta = 3: the last digit owns one row
    return 1 << 5, list(Q[:4]), list(P)              # "alpha2": alpha = 2, beta = 2


SHAPES = ["n16", "ragged", "alpha2"]
_RUNS = {}


def _run(oracle, pkg, name, scheme):
    key = (name, scheme)
    if key not in _RUNS:
        N, Q, P = _shape(pkg, name)
        st = ref.Setup(oracle, N, Q, P, scheme)
        gens = [5, pow(5, -1, 2 * N), 2 * N - 1]
        _RUNS[key] = (st, ref.run_all(st, ref.inputs(N, Q, P, 11, n_gens=len(gens)), gens))
    return _RUNS[key]


def _plain(st, p):
    """[rows, N] Montgomery residues -> lists of Python integers out of Montgomery form"""
    return [[int(v) * pow(R, -1, q) % q for v in row] for row, q in zip(p, st.moduli)]


def _ints(p):
    return [[int(v) for v in row] for row in p]


def _centred_rows(st, rows_ntt):
    """NTT-domain residues per row (Python integers) -> the coefficient-domain poly each row holds, centred; all rows must agree"""
    coeff = st.ctx.intt(np.array(rows_ntt, dtype=np.uint64))
    out = None
    for row, q in zip(coeff, st.moduli):
        c = [int(v) - q if int(v) > q // 2 else int(v) for v in row]
        assert out is None or c == out, "the rows do not hold one integer poly"
        out = c
    return out


def _noise_sum(e):
    """the centred integer sum of noise bytes [..., N] over all leading axes: sign 1 -> +c, sign 0 -> -c"""
    e = np.asarray(e).reshape(-1, e.shape[-1]).astype(np.int64)
    return [int(v) for v in np.where(e >> 7, e & 127, -(e & 127)).sum(axis=0)]


def _residual(st, key0, key1, s, target, i):
    """key0 + s key1 - P target w_i per row, NTT domain, all plain residues"""
    nQ, out = len(st.Q), []
    for j, q in enumerate(st.moduli):
        own = i * st.alpha <= j < min((i + 1) * st.alpha, nQ)
        p = st.Pbig % q if own else 0
        out.append([(a + x * b - p * t) % q for a, b, x, t in zip(key0[j], key1[j], s[j], target[j])])
    return out


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
@pytest.mark.parametrize("name", SHAPES)
def test_identities_in_python_integers(oracle, pkg, name, scheme):
    st, w = _run(oracle, pkg, name, scheme)
    n, N, h = N_PARTIES, st.N, st.N
    assert w["sk"].shape[0] == n
    s_mont = st.aggregate(list(w["sk"]))
    s = _plain(st, s_mont)
    s2 = [[x * x % q for x in row] for row, q in zip(s, st.moduli)]
    zero = [[0] * N for _ in st.moduli]
    # CKG: pk0 + s crs == sum e_i, exactly
    got = _centred_rows(st, _residual(st, _ints(w["pk0"]), _ints(w["crs"]), s, zero, 0))
    assert got == _noise_sum(w["ckg_e"])
    # RKG, three rounds
    bound = 2 * h * n * (MAG * n) + 2 * (MAG * n)
    worst = 0
    for i in range(st.beta):
        r = _centred_rows(st, _residual(st, _plain(st, w["rlk"][2 * i]), _plain(st, w["rlk"][2 * i + 1]), s, s2, i))
        worst = max(worst, max(abs(v) for v in r))
    print("RKG %s %s: largest residual %d, bound %d" % (name, scheme, worst, bound))
    assert 0 < worst <= bound
    # RKG, naive
    bound = MAG * n * (2 * h * h * n * n + 3 * h * n + 1)
    worst = 0
    for i in range(st.beta):
        r = _centred_rows(st, _residual(st, _plain(st, w["rlk_naive"][2 * i]), _plain(st, w["rlk_naive"][2 * i + 1]), s, s2, i))
        worst = max(worst, max(abs(v) for v in r))
    print("naive RKG %s %s: largest residual %d, bound %d" % (name, scheme, worst, bound))
    assert 0 < worst <= bound
    # RTG: key[i][0] + s key[i][1] - P pi(s) w_i == sum e_i, exactly
    for j, g in enumerate(w["gens"]):
        pis = _plain(st, st.ctx.permute_ntt(s_mont, g))
        for i in range(st.beta):
            r = _centred_rows(st, _residual(st, _plain(st, w["rot"][j][2 * i]), _plain(st, w["rot"][j][2 * i + 1]), s, pis, i))
            assert r == _noise_sum(w["rtg_e"][j][:, i]), (g, i)
            assert max(abs(v) for v in r) <= MAG * n
    # every stored residue is canonical
    for k in ("pk0", "rlk", "rlk_naive", "rot", "r1", "r2", "r3", "n1", "n2", "rtg", "ckg"):
        assert np.all(w[k] < np.array(st.moduli, dtype=np.uint64)[:, None]), k


def test_the_edge_bytes_are_in_the_inputs(pkg):
    N, Q, P = _shape(pkg, "ragged")
    d = ref.inputs(N, Q, P, 11)
    QP = np.array(Q + P, dtype=np.uint64)
    for k in ("ckg_e", "r1_e", "r2_e", "r3_e", "n1_e", "n2_e", "rtg_e"):
        flat = d[k].reshape(-1, N)
        assert list(flat[0, :6]) == [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80] and flat[-1, N - 1] == 0, k
    for k in ("sk_bits", "u_bits", "n1_bits", "n2_bits"):
        c, s = (x.reshape(-1, N >> 3) for x in d[k])
        pairs = {((int(c[0, 0]) >> b) & 1, (int(s[0, 0]) >> b) & 1) for b in range(8)}
        assert pairs == {(0, 0), (1, 0), (0, 1), (1, 1)} and np.all(c[-1] == 0xFF), k
    for a in (d["crs"], d["crp"][0], d["crp_rot"][0, 0]):
        assert np.all(a[:, 2] == 0) and np.array_equal(a[:, N - 1], QP - np.uint64(1))


@pytest.mark.parametrize("name", SHAPES)
def test_the_two_schemes_agree_where_their_lines_coincide(oracle, pkg, name):
    _, b = _run(oracle, pkg, name, "bfv")
    _, c = _run(oracle, pkg, name, "ckks")
    for k in ("sk", "u", "ckg", "pk0", "r1", "r1_sum", "r2", "r2_sum", "r3", "r3_sum", "rlk", "rtg", "rtg_sum", "rot"):
        assert np.array_equal(b[k], c[k]), k
    assert not np.array_equal(b["n1"], c["n1"])                      # dckks/relinkey_gen_naive.go:73-75
    # round two and the finalize of the naive protocol are the same lines: the same bits on the same round-one aggregate
    N, Q, P = _shape(pkg, name)
    sb, sc = ref.Setup(oracle, N, Q, P, "bfv"), ref.Setup(oracle, N, Q, P, "ckks")
    args = (b["n1_sum"], b["sk"][1], b["pk0"], b["crs"], b["n2_bits"][0][1], b["n2_bits"][1][1], b["n2_e"][1])
    assert np.array_equal(sb.naive_round2(*args), sc.naive_round2(*args))
    assert np.array_equal(sb.naive_key(b["n2_sum"]), sc.naive_key(b["n2_sum"]))


@pytest.mark.parametrize("name", SHAPES)
def test_the_dckks_naive_quirk_is_pinned(oracle, pkg, name):
    """dckks/relinkey_gen_naive.go:73-75: e[i][1] is the noise of [i][0], e[i][0] is lost, [i][1] = share_in + MRed(pk1, u_i)"""
    N, Q, P = _shape(pkg, name)
    sb, sc = ref.Setup(oracle, N, Q, P, "bfv"), ref.Setup(oracle, N, Q, P, "ckks")
    _, w = _run(oracle, pkg, name, "ckks")
    k = 1
    sk, pk0, pk1, e, bits = w["sk"][k], w["pk0"], w["crs"], w["n1_e"][k], (w["n1_bits"][0][k], w["n1_bits"][1][k])
    got = sc.naive_round1(sk, pk0, pk1, e, *bits)
    assert np.array_equal(got, w["n1"][k])
    swapped = e.copy()
    swapped[:, 0] = e[:, 1]
    want = sb.naive_round1(sk, pk0, pk1, swapped, *bits)
    assert np.array_equal(got[0::2], want[0::2])
    lost = e.copy()
    lost[:, 0] = 0x80 | 5                                            # the first draw changes nothing
    assert np.array_equal(sc.naive_round1(sk, pk0, pk1, lost, *bits), got)
    for i in range(sc.beta):
        t = sc.ternary_ntt(bits[0][i], bits[1][i])
        assert np.array_equal(got[2 * i + 1], sc.ctx.ewise("MUL_MONT", pk1, t)), i
    # onto whatever the share held: the reference accumulates; the device's convention is the freshly allocated (zero) share
    held = ref.uniform(np.random.default_rng(3), Q + P, N, 2 * sc.beta)
    again = sc.naive_round1(sk, pk0, pk1, e, *bits, share=held)
    assert np.array_equal(again[0::2], got[0::2])
    for i in range(sc.beta):
        assert np.array_equal(again[2 * i + 1], sc.ctx.ewise("ADD", held[2 * i + 1], got[2 * i + 1])), i


# ---- the device's fused order, in Python integers ----
def _cred(a, q):
    return a - q if a >= q else a


class _Dev:
    """what lr_setup.hip computes per coefficient: MRed, MForm and InvMForm are fully reduced, so each is its residue"""

    def __init__(self, st):
        self.st, self.rinv = st, [pow(R, -1, q) for q in st.moduli]

    def rows(self, f, *polys):
        out = []
        for j, q in enumerate(self.st.moduli):
            out.append([f(j, q, *vals) for vals in zip(*[p[j] for p in polys])])
        return np.array(out, dtype=np.uint64)

    def mred(self, j, q, x, y):
        return x * y * self.rinv[j] % q

    def noise(self, e_bytes):
        """launch_ckks_expand's operand: the q of (0, sign 0) written as 0; then the transform"""
        st = self.st
        x = ref.expand_gaussian(st.moduli, e_bytes, st.N)
        qs = np.array(st.moduli, dtype=np.uint64)[:, None]
        return _ints(st.ctx.ntt(np.where(x == qs, np.uint64(0), x)))

    def own(self, i, j):
        st = self.st
        return i * st.alpha <= j < min((i + 1) * st.alpha, len(st.Q))

    def times_p(self, j, q, s):
        pm = (self.st.Pbig % q) * R % q                                # MForm(P mod q)
        return self.mred(j, q, s, pm) * self.rinv[j] % q               # inv_mform(mred(s, pm))


@pytest.mark.parametrize("scheme", ["bfv", "ckks"])
@pytest.mark.parametrize("name", SHAPES)
def test_the_device_order_gives_the_restatements_bits(oracle, pkg, name, scheme):
    st, w = _run(oracle, pkg, name, scheme)
    D, k = _Dev(st), 2
    sk, u, crp = _ints(w["sk"][k]), _ints(w["u"][k]), [_ints(a) for a in w["crp"]]
    mulsub = lambda j, q, x, a, b: _cred(x + (q - D.mred(j, q, a, b)), q)
    add = lambda j, q, a, b: _cred(a + b, q)
    # CKG
    got = D.rows(lambda j, q, e, s, a: mulsub(j, q, e, s, a), D.noise(w["ckg_e"][k]), sk, _ints(w["crs"]))
    assert np.array_equal(got, w["ckg"][k])
    for i in range(st.beta):
        # round one: the digit add and the product with u in one pass
        f = lambda j, q, e, s, uu, a: mulsub(j, q, _cred(e + D.times_p(j, q, s), q) if D.own(i, j) else e, uu, a)
        assert np.array_equal(D.rows(f, D.noise(w["r1_e"][k][i]), sk, u, crp[i]), w["r1"][k][i]), ("r1", i)
        # round two: both outputs from one read of sk
        r1 = _ints(w["r1_sum"][i])
        f0 = lambda j, q, r, s, e: add(j, q, D.mred(j, q, r, s), e)
        f1 = lambda j, q, e, s, a: add(j, q, e, D.mred(j, q, s, a))
        assert np.array_equal(D.rows(f0, r1, sk, D.noise(w["r2_e"][k][i][0])), w["r2"][k][2 * i]), ("r2", i, 0)
        assert np.array_equal(D.rows(f1, D.noise(w["r2_e"][k][i][1]), sk, crp[i]), w["r2"][k][2 * i + 1]), ("r2", i, 1)
        # round three: u - sk in registers
        f = lambda j, q, e, uu, s, r: add(j, q, e, D.mred(j, q, _cred((uu + q) - s, q), r))
        assert np.array_equal(D.rows(f, D.noise(w["r3_e"][k][i]), u, sk, _ints(w["r2_sum"][2 * i + 1])), w["r3"][k][i]), ("r3", i)
        # the key step: Add and both MForms
        f = lambda j, q, a, b: _cred(a + b, q) * R % q
        assert np.array_equal(D.rows(f, _ints(w["r2_sum"][2 * i]), _ints(w["r3_sum"][i])), w["rlk"][2 * i]), ("rlk", i, 0)
        assert np.array_equal(D.rows(lambda j, q, a: a * R % q, _ints(w["r2_sum"][2 * i + 1])), w["rlk"][2 * i + 1]), ("rlk", i, 1)
        # naive round one, with the dckks quirk as the kernel takes it: e[i][1] for [i][0], a zero for [i][1]
        t = _ints(st.ternary_ntt(w["n1_bits"][0][k][i], w["n1_bits"][1][k][i]))
        e0, e1 = D.noise(w["n1_e"][k][i][0]), D.noise(w["n1_e"][k][i][1])
        pk0, pk1 = _ints(w["pk0"]), _ints(w["crs"])
        quirk = scheme == "ckks"
        f0 = lambda j, q, e, s, p, tt: add(j, q, _cred(e + D.times_p(j, q, s), q) if D.own(i, j) else e, D.mred(j, q, p, tt))
        f1 = lambda j, q, e, p, tt: add(j, q, 0 if quirk else e, D.mred(j, q, p, tt))
        assert np.array_equal(D.rows(f0, e1 if quirk else e0, sk, pk0, t), w["n1"][k][2 * i]), ("n1", i, 0)
        assert np.array_equal(D.rows(f1, e1, pk1, t), w["n1"][k][2 * i + 1]), ("n1", i, 1)
        # naive round two
        t = _ints(st.ternary_ntt(w["n2_bits"][0][k][i], w["n2_bits"][1][k][i]))
        f = lambda j, q, r, s, p, tt, e: add(j, q, add(j, q, D.mred(j, q, r, s), D.mred(j, q, p, tt)), e)
        for c, pk in enumerate((pk0, pk1)):
            got = D.rows(f, _ints(w["n1_sum"][2 * i + c]), sk, pk, t, D.noise(w["n2_e"][k][i][c]))
            assert np.array_equal(got, w["n2"][k][2 * i + c]), ("n2", i, c)
        # the RTG share: the Galois gather inside the pass
        for g_i, g in enumerate(w["gens"]):
            index = [int(v) for v in st.ctx.permute_ntt_index(g, 1)]
            a = _ints(w["crp_rot"][g_i][i])
            e = D.noise(w["rtg_e"][g_i][k][i])
            got = []
            for j, q in enumerate(st.moduli):
                row = []
                for pos in range(st.N):
                    x = e[j][pos]
                    if D.own(i, j):
                        x = _cred(x + D.times_p(j, q, sk[j][index[pos]]), q)
                    row.append(mulsub(j, q, x, a[j][pos], sk[j][pos]) * R % q)
                got.append(row)
            assert np.array_equal(np.array(got, dtype=np.uint64), w["rtg"][g_i][k][i]), ("rtg", g, i)


@pytest.mark.parametrize("kg_scheme", ["ckks", "bfv"])
@pytest.mark.parametrize("name", SHAPES)
def test_the_rtg_share_is_the_key_generators_evakey_with_mform_crp(oracle, pkg, name, kg_scheme):
    """for one party, replace newSwitchingKey's uniform half a by MForm(crp): genrotKey's evakey[i][0] is then RTG's share[i] bit for bit
    (every step of both is fully reduced, and MForm is the exact multiplication by 2^64) -- measured here, not argued"""
    st, w = _run(oracle, pkg, name, "bfv")
    N, Q, P = _shape(pkg, name)
    kg = keygen_ref.KeyGenerator(oracle, N, Q, P, kg_scheme)
    for g_i, g in enumerate(w["gens"]):
        crp, e = w["crp_rot"][g_i], w["rtg_e"][g_i][0]
        a = np.stack([st.ctx.ewise("MFORM", x) for x in crp])
        key = kg.gen_rot_key(w["sk"][0], g, e, a)
        assert np.array_equal(key[0::2], w["rtg"][g_i][0]), g
        assert np.array_equal(key, st.rtg_key(w["rtg"][g_i][0], crp)), g        # and Finalize of the lone share is the whole key
