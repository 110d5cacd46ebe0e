"""The shape generator of the handles' fuzz (tests/handle_fuzz_shapes.py), without a device.

Determinism: draw(family, seed) gives the same dict twice.  The move of the two modulus pools out of tests/test_gpu_fuzz.py changed no
shape of the eight older fuzz families: three seeds of each are replayed against values recorded before the move.  Coverage: over the
committed seeds of every family the conditions of coverage() hold -- the short last digit, |Q| < alpha, the levels, the modulus classes,
the bands of degrees, the option sets, both forms of the randomness, batches below max_batch, keys of their own, wrapped outputs, the mask
word counts -- so that the device tests' reach can be read off here.  Meaning: on every committed seed with logN <= 6 the restatement the
device is compared with is checked with Python integers -- the public-key identity, every switching key digit by digit with its noise
recovered, a CKS share chain that decrypts to the plaintext within 1, Refresh returning the plaintext exactly (CKKS) or after the
rounding (BFV, where Q leaves room for t) -- which pins the reference on the short-digit and mixed-moduli shapes."""
import numpy as np
import pytest

import handle_fuzz_shapes as shapes
from bfv_encryptor_ref import expand_gaussian
from test_oracle_collective import _crt, _negacyclic, _plain_coeffs, _prod, _signed_noise
from test_oracle_keygen import R, _check_identity, _ints

SEEDS = range(shapes.SEEDS)

# ---- the older families draw what they drew ----------------------------------------------------------------------------------------------
# seed -> the head of the shape (and the moduli where a pool is used), recorded before the pools moved into handle_fuzz_shapes.py
RECORDED = {
    "ntt_and_elementwise": {0: [3, 4, 4, 2, [2305843009213693921, 1152921504066306049, 144115188075854689, 1099511627873]],
                            13: [3, 5, 2, 0, [576460752586407937, 1152921504050839553, 1152921504093306881, 1152921504096452609, 144115188075854689]],
                            27: [16, 4, 1, 0, [2305843009211596801, 1125899908022273, 576460752580902913, 576460752573431809]]},
    "basis_extension_and_rescale": {0: [5, 5, 1, 2, [17179869697, 1152921504050839553, 144115188075853249, 1152921504606850369, 4294966657, 144115188075856001]],
                                    4: [10, 6, 2, 1, [4294991873, 576460752573431809, 1152921504093306881, 576460752585490433, 1152921504078364673, 4294957057,
                                                      1152921504050839553, 1152921504066306049]],
                                    9: [12, 2, 2, 2, [8589852673, 144115188075814913, 1152921504606830593, 1152921504057917441]]},
    "key_switch": {0: [10, 5, 2, 1, 0], 7: [12, 5, 1, 3, 2], 15: [16, 6, 1, 2, 1]},
    "dual_kernel": {0: [12, 7, 2, 6, [72057594038149121, 70368743669761, 8589852673, 1125899906949121, 4294991873, 70368744210433, 17179967489]],
                    5: [12, 7, 3, 2, [4294828033, 1073815553, 70368744210433, 1125899906990081, 35184372121601, 1099511922689, 8589852673]],
                    11: [13, 4, 1, 1, [70368744570881, 1125899906990081, 35184372121601, 1099512004609]]},
    "mulrelin_rescale": {0: [12, 5, 1, 2, 2], 3: [15, 4, 2, 1, 1], 7: [14, 6, 4, 4, 1]},
    "rotation_encrypt_decrypt": {0: [10, 6, 1, 3, 2], 5: [5, 6, 3, 1, 3], 11: [13, 5, 4, 2, 2]},
    "moddown_divfloor_permute": {2: [5, 5, 1, 3, 3, [8589934721, 576460752580902913, 4294967681, 8589933377, 1152921504078364673, 1152921504050839553]],
                                 5: [5, 3, 3, 3, 1, [576460752585490433, 1152921504053723137, 1152921504050839553, 1125899906843009, 1099511628161, 70368744177601]],
                                 11: [16, 7, 4, 2, 3, [17180262401, 576460752573431809, 576460752585490433, 1152921504066306049, 1152921504606584833,
                                                       1152921504078364673, 4293918721, 8589279233, 70368740769793, 576460752586407937, 1125899911168001]]},
    "bfv_pipelines": {0: [6, 2, 1, 1], 5: [9, 3, 1, 3], 9: [13, 3, 1, 3]},
}


def _replay(pkg, family, seed):
    """the draws at the head of tests/test_gpu_fuzz.py's bodies, in their order, with the pools as that module sees them"""
    import test_gpu_fuzz as F
    i = lambda rng, lo, hi: int(rng.integers(lo, hi))
    if family == "ntt_and_elementwise":
        rng = np.random.default_rng(1000 + seed)
        logn = i(rng, 1, 15) if seed < 24 else 15 + seed % 2
        limbs = i(rng, 1, 7)
        batch, level = i(rng, 1, 5), i(rng, 0, limbs)
        return [logn, limbs, batch, level, F._moduli(pkg, rng, max(logn, 4), limbs)]
    if family == "basis_extension_and_rescale":
        rng = np.random.default_rng(2000 + seed)
        logn, nq, np_, batch = i(rng, 3, 13), i(rng, 1, 9), i(rng, 1, 5), i(rng, 1, 4)
        return [logn, nq, np_, batch, F._moduli(pkg, rng, max(logn, 4), nq + np_)]
    if family == "key_switch":
        rng = np.random.default_rng(3000 + seed)
        logn = i(rng, 4, 13) if seed < 8 else 13 + (seed % 4)
        nq, np_, batch = i(rng, 2, 10), i(rng, 1, 5), i(rng, 1, 4)
        return [logn, nq, np_, batch, i(rng, 0, nq)]
    if family == "dual_kernel":
        rng = np.random.default_rng(4000 + seed)
        logn, limbs, batch = 12 + seed % 5, i(rng, 1, 8), i(rng, 1, 4)
        return [logn, limbs, batch, i(rng, 0, limbs), F._ckks_size_moduli(pkg, rng, logn, limbs)]
    if family == "mulrelin_rescale":
        rng = np.random.default_rng(5000 + seed)
        nq, np_ = i(rng, 3, 9), i(rng, 1, 5)
        return [12 + seed % 5, nq, np_, i(rng, 1, nq), i(rng, 1, 4)]
    if family == "rotation_encrypt_decrypt":
        rng = np.random.default_rng(6000 + seed)
        logn = i(rng, 4, 13) if seed < 6 else 12 + seed % 5
        nq, np_, batch = i(rng, 2, 9), i(rng, 1, 5), i(rng, 1, 4)
        return [logn, nq, np_, batch, i(rng, 0, nq)]
    if family == "moddown_divfloor_permute":
        rng = np.random.default_rng(7000 + seed)
        logn = i(rng, 4, 13) if seed < 6 else 11 + seed % 6
        nq, np_, batch = i(rng, 2, 9), i(rng, 1, 5), i(rng, 1, 4)
        level = i(rng, 0, nq)
        assert seed % 3 == 2                                             # the seeds that draw from the pool
        return [logn, nq, np_, batch, level, F._moduli(pkg, rng, max(logn, 4), nq + np_)]
    rng = np.random.default_rng(8000 + seed)                             # bfv_pipelines
    Nfull, Qf, Pf, _ = pkg.params.bfv_moduli(("PN12QP109", "PN13QP218", "PN14QP438", "PN15QP880")[seed % 4])
    top = Nfull.bit_length() - 1
    logn = i(rng, 6, top + 1) if seed < 6 else min(top, 12 + seed % 4)
    nq = min(i(rng, 2, len(Qf) + 1) if len(Qf) > 2 else len(Qf), 7)
    return [logn, nq, i(rng, 1, len(Pf) + 1), i(rng, 1, 4)]


@pytest.mark.parametrize("family", list(RECORDED))
def test_the_older_families_draw_the_shapes_they_drew(pkg, family):
    for seed, want in RECORDED[family].items():
        assert _replay(pkg, family, seed) == want, (family, seed)


def test_the_pools_are_the_packages_own(pkg):
    """handle_fuzz_shapes reads the package's params module through tests/limit_moduli.py: the same primes either way"""
    for logn in (4, 12, 15):
        for pool in (shapes._moduli, shapes._ckks_size_moduli):
            a = pool(pkg, np.random.default_rng(logn), logn, 5)
            assert a == pool(shapes._Params, np.random.default_rng(logn), logn, 5)


# ---- determinism and coverage -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", shapes.FAMILIES)
def test_draw_is_deterministic(family):
    for seed in list(SEEDS) + [977]:
        a, b = shapes.draw(family, seed), shapes.draw(family, seed)
        assert a == b and repr(a) == repr(b)
        N = 1 << a["logn"]
        assert 1 <= len(a["Q"]) <= 8 and len(a["P"]) <= 4 and 1 <= a["batch"] <= 5 and a["batch"] <= a["max_batch"]
        assert a["logn"] >= shapes.MIN_LOGN.get(family, 3) and a["logn"] < 16                       # no 2^16 seed: the structured tests have it
        assert all(q % (2 * N) == 1 and q < 1 << 61 for q in a["Q"] + a["P"]) and len(set(a["Q"] + a["P"])) == len(a["Q"] + a["P"])
        assert 0 <= a["level"] < len(a["Q"])
        if a["t"]:
            assert a["t"] % (2 * N) == 1                                                            # NTT-friendly at the drawn N
        assert (a["expect_refusal"] is not None) == (not a["P"] and family in shapes.EMPTY_P)
    assert shapes.draw(family, 0) != shapes.draw(family, 1)
    for seed, logn in shapes.PINNED.items():
        d = shapes.draw(family, seed)
        assert d["logn"] == logn and len(d["Q"]) <= 2 and len(d["P"]) == (0 if family in shapes.NO_P else 1) and d["batch"] == 1
        if family == "ckks_encoder":
            assert d["slots"] <= 64


def coverage(family, cases):
    """condition -> (seeds that meet it, seeds needed)"""
    out = {}

    def need(name, k, pred):
        out[name] = (sum(1 for d in cases if pred(d)), k)
    alpha, nq, qp = (lambda d: len(d["P"])), (lambda d: len(d["Q"])), (lambda d: d["Q"] + d["P"])
    if family in ("keygen", "setup", "collective"):                      # the digit loops' break
        need("a short last digit", 3, lambda d: alpha(d) and nq(d) % alpha(d))
        need("|Q| < alpha", 1, lambda d: nq(d) < alpha(d))
        need("a short last digit behind full ones", 2, lambda d: alpha(d) and nq(d) % alpha(d) and nq(d) > alpha(d))
        # ... each on the fused shape (the kernels' own break) and on the call-by-call shape of no_epilogue (the host's row bounds)
        for shape, pick in (("fused", lambda d: d["options"] != "no_epilogue"), ("call-by-call", lambda d: d["options"] == "no_epilogue")):
            need("a short last digit behind full ones, " + shape, 1, lambda d, pick=pick: pick(d) and alpha(d) and nq(d) % alpha(d) and nq(d) > alpha(d))
            need("|Q| < alpha, " + shape, 1, lambda d, pick=pick: pick(d) and nq(d) < alpha(d))
    if family in shapes.HAS_LEVEL:
        lvl = (lambda d: d["level_start"]) if family == "refresh" else (lambda d: d["level"])
        need("level 0", 2, lambda d: lvl(d) == 0)
        need("the top level", 1, lambda d: lvl(d) == nq(d) - 1)
        need("the top level of several limbs", 1, lambda d: lvl(d) == nq(d) - 1 and nq(d) > 1)
        need("a level between the ends", 2, lambda d: 0 < lvl(d) < nq(d) - 1)
        if family != "ckks_encoder":
            need("level + 1 not a multiple of alpha", 2, lambda d: alpha(d) and (lvl(d) + 1) % alpha(d))
    need("a 61-bit prime", 2, lambda d: any(q >= 1 << 60 for q in qp(d)))
    need("a prime <= 2^34", 2, lambda d: any(q <= 1 << 34 for q in qp(d)))
    need("a prime below 2^46 next to one above 2^57", 2, lambda d: any(q < 1 << 46 for q in qp(d)) and any(q > 1 << 57 for q in qp(d)))
    need("logN <= 7", 3, lambda d: d["logn"] <= 7)
    need("logN 8 .. 11", 3, lambda d: 8 <= d["logn"] <= 11)
    need("logN 12 or 13", 2, lambda d: d["logn"] in (12, 13))
    need("logN 14", 1, lambda d: d["logn"] == 14)
    need("logN 15", 1, lambda d: d["logn"] == 15)
    # the two large degrees are there for the assembly kernels: one seed on the fused shape, one on the call-by-call shape, none with no_asm
    need("a large degree on the fused shape, assembly on", 1, lambda d: d["logn"] >= 14 and d["options"] == "default")
    need("a large degree on the call-by-call shape, assembly on", 1, lambda d: d["logn"] >= 14 and d["options"] == "no_epilogue")
    for o in shapes.OPTION_SETS:
        need("options " + o, 2, lambda d, o=o: d["options"] == o)
    need("options on the contexts only", 2, lambda d: d["options_on"] == "context")
    need("options on the handle as well", 2, lambda d: d["options_on"] == "both")
    for f in ("host", "device"):
        need("randomness in " + f + " form", 3, lambda d, f=f: d["form"] == f)
    need("max_batch > batch", 3, lambda d: d["max_batch"] > d["batch"])
    if family not in shapes.NO_P:
        need("keys of their own", 3, lambda d: d["own_keys"] and d["batch"] > 1)
    need("a wrapped output", 3, lambda d: any(o is not None for o in d["out"]))
    # a kernel that wrote max_batch members would show in the members behind a wrapped output of a smaller batch
    need("a wrapped first output with max_batch > batch", 2, lambda d: d["out"][0] is not None and d["max_batch"] > d["batch"])
    if family == "refresh":
        W = lambda d: shapes.mask_words(d["Q"], d["level_start"])
        need("one mask word", 2, lambda d: W(d) == 1)
        need("two mask words", 2, lambda d: W(d) == 2)
        need("three or more mask words", 2, lambda d: W(d) >= 3)
        need("more than four digits in Recode", 1, lambda d: d["level_start"] + 1 > 4)
    return out


@pytest.mark.parametrize("family", shapes.FAMILIES)
def test_the_committed_seeds_cover_what_they_are_there_for(family):
    cases = [shapes.draw(family, seed) for seed in SEEDS]
    missing = {k: v for k, v in coverage(family, cases).items() if v[0] < v[1]}
    assert not missing, (family, missing)
    assert sum(1 for d in cases if d["expect_refusal"]) <= 1             # at most one committed seed per family is an expected refusal
    assert [d["logn"] for d in cases if d["seed"] in shapes.PINNED] == [14, 15] and all(d["logn"] <= 13 for d in cases if d["seed"] not in shapes.PINNED)


def test_the_inputs_carry_the_edge_decisions():
    rng = np.random.default_rng(1)
    e = shapes.noise(rng, (3, 2, 16))
    assert set(shapes.NOISE_EDGES) <= set(int(v) for v in e.reshape(-1)) and (e & 127).max() == 127
    c, s = shapes.planes(rng, (4, 2))
    pairs = {(int(a), int(b)) for a, b in zip(c.reshape(-1), s.reshape(-1))}
    assert (0b10101010, 0b11001100) in pairs and (0xFF in c.reshape(4, 2).min(axis=1) or 0xFF in s.reshape(4, 2).min(axis=1))
    Q = [shapes.lm.below(61, 4), shapes.lm.below(32, 4), shapes.lm.above(46, 4)]
    a = shapes.uniform(rng, Q, 16, 3)
    assert any((a[k, :, j] == 0).all() for k in range(3) for j in range(16))
    assert any((a[k, :, j] == np.array(Q, dtype=np.uint64) - np.uint64(1)).all() for k in range(3) for j in range(16))
    for ls, words in ((0, 1), (1, 2), (2, 3)):
        m = shapes.refresh_masks(rng, Q, ls, 32)
        top = 1 << (64 * words - 1)
        assert shapes.mask_words(Q, ls) == words and {0, 1, -1, top - 1, -top, 3 * Q[0]} <= set(m) and all(-top <= v < top for v in m)
        v = shapes.recode_integers(rng, Q, ls, 16)
        Qls = shapes.product(Q[:ls + 1])
        assert {0, Qls - 1, (Qls - 1) // 2, (Qls + 1) // 2} <= set(v) and all(0 <= x < Qls for x in v)


@pytest.mark.parametrize("seed", SEEDS)
def test_bfv_encoder_restatement_round_trip(oracle, seed):
    """Decode(Encode(v)) = v mod t slot for slot wherever Q > 2 t^2 (the scaling's error m (Q mod t) / Q is below 1 / 2 there), and the
    committed seeds have such shapes"""
    c = shapes.reference(oracle, shapes.draw("bfv_encoder", seed))
    nv = c["n_values"]
    if c["round_trip_exact"]:
        assert np.array_equal(c["dec_back"][:, :nv], c["u"] % np.uint64(c["t"])) and not c["dec_back"][:, nv:].any()
    assert sum(1 for s in SEEDS if shapes.product(shapes.draw("bfv_encoder", s)["Q"]) > 2 * shapes.draw("bfv_encoder", s)["t"] ** 2) >= 6


# ---- the meaning of the restatement on the small seeds, with Python integers ------------------------------------------------------------
def _small(family, logn=6):
    return [seed for seed in SEEDS if shapes.draw(family, seed)["logn"] <= logn]


def _centred(x, M):
    x %= M
    return x - M if x > M // 2 else x


def _ckks_room(d):
    """what Q_levelStart / 2 leaves for the plaintext beside a party's mask (below Q_ls / 6) and the noise"""
    Qls = _prod(d["Q"][:d["level_start"] + 1])
    return Qls // 2 - max(Qls // 6, 1) - 256


def _bfv_too_small(d):
    """Delta / 2 is no larger than the noise the protocol adds (t from the mask's wrap, N from the rounding of crs / P): nothing to decode"""
    return _prod(d["Q"]) < 4 * d["t"] * (d["t"] + (1 << d["logn"]) + 256)


def test_small_seeds_exist_for_every_checked_family():
    for family in ("keygen", "setup", "collective", "refresh"):
        assert _small(family), family
    # ... and they reach the shapes the check is there for
    # ... and the refresh check runs both of its halves: a Q_ls that leaves room for the plaintext, a Q that leaves room for t
    cases = [shapes.draw("refresh", s) for s in _small("refresh")]
    assert any(_ckks_room(d) >= 1 for d in cases), "no small refresh seed runs the CKKS check"
    assert any(d["P"] and not _bfv_too_small(d) for d in cases), "no small refresh seed runs the BFV check"
    for f in ("keygen", "setup"):                                       # (the row-by-row identities cost N, not N^2: up to 2^8 there)
        cases = [shapes.draw(f, s) for s in _small(f, 8)]
        assert any(d["P"] and len(d["Q"]) % len(d["P"]) and len(d["Q"]) > len(d["P"]) for d in cases), (f, "no small seed has a short last digit")
    assert any(len(d["Q"]) < len(d["P"]) for f in ("keygen", "setup", "collective") for d in (shapes.draw(f, s) for s in _small(f, 8)))


@pytest.mark.parametrize("seed", _small("keygen", 8))
def test_keygen_restatement_in_python_integers(oracle, seed):
    """pk0 + sk pk1 R^-1 + NTT(e) == 0, and every switching key row by row: evk[i][0] + a_i skOut R^-1 - [row in digit i] P skIn == NTT(e_i) R"""
    c = shapes.reference(oracle, shapes.draw("keygen", seed))
    kg, n = c["ref"], c["n"]
    for b in range(n):
        sk = c["sk"][c["key"](b)]
        ntt_e = kg.ctx.ntt(expand_gaussian(kg.moduli, c["pk_e"][b], c["N"]))
        for j, q in enumerate(kg.moduli):
            r_inv = pow(R, -1, q)
            for x, s, a1, en in zip(_ints(c["pk0"][b][j]), _ints(sk[j]), _ints(c["pk1"][b][j]), _ints(ntt_e[j])):
                assert (x + s * a1 * r_inv + en) % q == 0 and 0 < x <= q, (seed, b, j)
    if not c["nP"]:
        return
    power = c["sk"][0]
    for k in range(n):
        _check_identity(kg, c["swk"][k], c["sk_in"][c["key"](k)], c["sk_out"][c["key"](k)], c["e"][k], c["a"][k])
        power = kg.ctx.ewise("MUL_MONT", power, c["sk"][0])
        _check_identity(kg, c["rlk"][k], power, c["sk"][0], c["e"][k], c["a"][k])
        _check_identity(kg, c["rot"][k], kg.ctx.permute_ntt(c["sk"][0], c["gens"][k]), c["sk"][0], c["e"][k], c["a"][k])


@pytest.mark.parametrize("seed", _small("setup", 8))
def test_setup_restatement_in_python_integers(oracle, seed):
    """the CKG share is a public-key share, and one party's RTG share, finalized, is a rotation key: keygen's identity holds for it digit by
    digit (member 2 i + 1 = MForm(crp[i]) stands for a_i)"""
    import keygen_ref
    c = shapes.reference(oracle, shapes.draw("setup", seed))
    st, n, w = c["ref"], c["n"], c["want"]
    for k in range(n):
        sk, ntt_e = c["sk"][c["key"](k)], st.ctx.ntt(expand_gaussian(st.moduli, c["ckg_e"][k], c["N"]))
        for j, q in enumerate(st.moduli):
            r_inv = pow(R, -1, q)
            for x, s, a1, en in zip(_ints(w["ckg"][k][j]), _ints(sk[j]), _ints(c["crs"][j]), _ints(ntt_e[j])):
                assert (x + s * a1 * r_inv - en) % q == 0 and x < q, (seed, k, j)
    if not c["nP"]:
        return
    kg = keygen_ref.KeyGenerator(oracle, c["N"], c["Q"], c["P"], "bfv")
    a = np.stack([st.ctx.ewise("MFORM", c["crp"][i]) for i in range(c["beta"])])
    for k in range(n):
        key = st.rtg_key(w["rtg"][k], c["crp"])
        _check_identity(kg, key, st.ctx.permute_ntt(c["sk"][0], c["gens"][k]), c["sk"][0], c["rtg_e"][k], a)


@pytest.mark.parametrize("seed", _small("collective"))
def test_cks_chain_decrypts_to_the_plaintext(oracle, seed):
    """a ciphertext (m - c1 s_in, c1) at the drawn level, one CKS share added to its first component, decrypted under s_out: m, within 1
    per coefficient.  The share is round((P c1 (s_in - s_out) + e) / P) with |e| <= 127 < P / 2, so that the noise divides away; the 1 is
    the ModDown's float correction (tests/test_oracle_collective.py).  Both schemes' shares, Python integers throughout."""
    c = shapes.reference(oracle, shapes.draw("collective", seed))
    N, Q, nQ, col = c["N"], c["Q"], c["nQ"], c["ref"]
    rng = np.random.default_rng(seed)
    for scheme, level in (("ckks", c["level"]), ("bfv", nQ - 1)):
        Ql = Q[:level + 1]
        M, cl = _prod(Ql), oracle.Context(N, Ql)
        for b in range(c["n"]):
            s_in = _plain_coeffs(oracle, N, Ql, c["sk_in"][c["key"](b)][:level + 1])
            s_out = _plain_coeffs(oracle, N, Ql, c["sk_out"][c["key"](b)][:level + 1])
            rows = c["c1"][b][:level + 1]
            c1 = _crt(cl.intt(np.ascontiguousarray(rows)) if scheme == "ckks" else rows, Ql)
            m = [int(v) for v in rng.integers(0, 1 << 20, N)]
            c0 = [(x - y) % M for x, y in zip(m, _negacyclic(c1, s_in, M))]
            share = c[scheme + "_cks"][b]
            share = _crt(cl.intt(share) if scheme == "ckks" else share, Ql)
            phase = [(x + h + y) % M for x, h, y in zip(c0, share, _negacyclic(c1, s_out, M))]
            assert max(abs(_centred(p - x, M)) for p, x in zip(phase, m)) <= 1, (seed, scheme, b)


@pytest.mark.parametrize("seed", _small("refresh"))
def test_refresh_returns_the_plaintext(oracle, seed):
    """CKKS: a ciphertext of m at levelStart with |m + mask + e0| < Q_ls / 2, one party's shares, Finalize: (out0, crs) decrypts over all of Q
    to m + e0 - e1 exactly -- no step divides.  BFV, where Q >= 4 t (t + N + 256) leaves room: Delta m + v is refreshed to a ciphertext that
    decrypts to m after the rounding by t / Q."""
    c = shapes.reference(oracle, shapes.draw("refresh", seed))
    N, Q, nQ, ls, r = c["N"], c["Q"], c["nQ"], c["level_start"], c["ref"]
    Qls, Qall = _prod(Q[:ls + 1]), _prod(Q)
    rng = np.random.default_rng(seed)
    cQ, cl = oracle.Context(N, Q), oracle.Context(N, Q[:ls + 1])
    e = [_signed_noise(c["e"][0, 0]), _signed_noise(c["e"][1, 0])]
    sk = c["sk"][0][:nQ]
    s = _plain_coeffs(oracle, N, Q, sk)
    # the mask a party draws is below Q_ls / 2 nParties; the plaintext fills what three parties leave
    bound = max(Qls // 6, 1)
    mask = [_centred(int.from_bytes(rng.bytes(8 * nQ + 8), "little") % bound, bound) for _ in range(N)]
    room = max(_ckks_room(c), 1)
    m = [_centred(int.from_bytes(rng.bytes(8 * nQ + 8), "little") % room, room) for _ in range(N)]
    c1_rows = c["c1"][0][:ls + 1]
    c1 = _crt(cl.intt(np.ascontiguousarray(c1_rows)), Q[:ls + 1])
    c0 = [(x - y) % Qls for x, y in zip(m, _negacyclic(c1, [v % Qls for v in s], Qls))]
    c0_rows = cl.ntt(np.array([[v % q for v in c0] for q in Q[:ls + 1]], dtype=np.uint64))
    dec, rec = r.ckks_gen_shares(ls, sk, c["c1"][0], c["crs"][0], mask, c["e"][0, 0], c["e"][1, 0])
    out0 = r.ckks_finalize(ls, c0_rows, dec, rec)
    crs = _crt(cQ.intt(c["crs"][0]), Q)
    phase = [(x + y) % Qall for x, y in zip(_crt(cQ.intt(out0), Q), _negacyclic(crs, s, Qall))]
    if _ckks_room(c) >= 1:
        assert [_centred(p, Qall) for p in phase] == [x + a - b for x, a, b in zip(m, e[0], e[1])], (seed, "ckks")
    if not c["bfv"]:
        return
    t, P = c["t"], c["P"]
    if _bfv_too_small(c):
        return
    delta = Qall // t
    sk_qp = c["sk"][0]
    m = [int(v) for v in rng.integers(0, t, N)]
    v = [int(x) for x in rng.integers(-64, 65, N)]
    c1 = _crt(c["c1"][0], Q)
    c0 = [(delta * x + n - y) % Qall for x, n, y in zip(m, v, _negacyclic(c1, s, Qall))]
    c0_rows = np.array([[x % q for x in c0] for q in Q], dtype=np.uint64)
    dec, rec = r.bfv_gen_shares(sk_qp, c["c1"][0], c["crs_qp"][0], c["mask_bfv"][0], c["e"][0, 0], c["e"][1, 0])
    out = r.bfv_finalize(c0_rows, c["crs_qp"][0], dec, rec)
    phase = [(x + y) % Qall for x, y in zip(_crt(out[0], Q), _negacyclic(_crt(out[1], Q), s, Qall))]
    assert [((2 * t * p + Qall) // (2 * Qall)) % t for p in phase] == m, (seed, "bfv")
    assert max(abs(_centred(p - delta * x, Qall)) for p, x in zip(phase, m)) < delta // 2
