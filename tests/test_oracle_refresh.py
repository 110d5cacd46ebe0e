"""The restatement of the collective Refresh (tests/refresh_ref.py) on the CPU: identities against Python integers, the device's default
shapes and word arithmetic restated in their order giving the restatement's bits, and three-party chains at PN12QP109."""
import numpy as np
import pytest

import keygen_ref
import refresh_ref as ref


def _small(pkg, scheme):
    """N = 2^4, 2 + 1 limbs of Qi60 / Pi60"""
    return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])


def _edge_masks(Q, level_start, N):
    """0, +-1, +-(2^64 - 1), +-2^64, the largest and smallest W-word values, a multiple of q_i, then whatever fits of a fixed sequence"""
    W = ref.mask_words(Q, level_start)
    top = 1 << (64 * W - 1)
    edges = [0, 1, -1, (1 << 64) - 1, -((1 << 64) - 1), 1 << 64, -(1 << 64), top - 1, -top, 3 * Q[0], -5 * Q[-1]]
    edges = [v for v in edges if -top <= v < top]
    rng = np.random.default_rng(11)
    more = [int.from_bytes(rng.bytes(8 * W), "little") - top for _ in range(max(0, N - len(edges)))]
    return (edges + more)[:N], W


def _ckks_case(oracle, pkg, N, Q, seed=5):
    rng = np.random.default_rng(seed)
    sk = keygen_ref.uniform(rng, Q, N)          # any residues serve the identities
    c1, crs = keygen_ref.uniform(rng, Q, N), keygen_ref.uniform(rng, Q, N)
    e = ref.regular_bytes(rng, (2, N))
    e[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
    e[1, N - 1] = 0
    return sk, c1, crs, e


@pytest.mark.parametrize("level_start", [0, 1])
def test_mask_words_reduce_as_the_integers_they_are(pkg, level_start):
    N, Q, _ = _small(pkg, "ckks")
    for moduli in (Q, list(pkg.params.ckks_moduli("PN13QP218")[1])):
        for ls in sorted({level_start, len(moduli) - 1}):
            masks, W = _edge_masks(moduli, ls, 16)
            planes = pkg.sampling.mask_word_planes(masks, W)
            assert planes.shape == (W, 16) and planes.dtype == np.uint64
            for j, v in enumerate(masks):
                back = sum(int(planes[w, j]) << (64 * w) for w in range(W))
                assert (back - (1 << (64 * W)) if back >> (64 * W - 1) else back) == v
                for q in moduli:
                    assert ref.reduce_words(planes[:, j], q) == v % q, (v, q)
    with pytest.raises(ValueError):
        pkg.sampling.mask_word_planes([1 << 63], 1)
    assert pkg.sampling.mask_word_planes([[1, 2], [3, 4]], 2).shape == (2, 2, 2)


@pytest.mark.parametrize("level_start", [0, 1])
def test_a_share_plus_its_counterpart_cancels_the_mask(oracle, pkg, level_start):
    N, Q, P = _small(pkg, "ckks")
    r = ref.Refresh(oracle, N, Q)
    sk, c1, crs, e = _ckks_case(oracle, pkg, N, Q)
    masks, _ = _edge_masks(Q, level_start, N)
    L1 = level_start + 1
    # the same c1 and crs, the same noise: what is left of dec + rec is nothing
    crs_same = crs.copy()
    crs_same[:L1] = c1[:L1]
    dec, rec = r.ckks_gen_shares(level_start, sk, c1, crs_same, masks, e[0], e[0])
    assert not r.cQ.ewise("REDUCE", r.cQ.ewise("ADD", dec, rec[:L1])).any()
    # against no mask: the difference is NTT(mask mod q_i) on either share
    dec0, rec0 = r.ckks_gen_shares(level_start, sk, c1, crs, [0] * N, e[0], e[1])
    dec, rec = r.ckks_gen_shares(level_start, sk, c1, crs, masks, e[0], e[1])
    m = r.cQ.ntt(np.array([[v % q for v in masks] for q in Q], dtype=np.uint64))
    assert np.array_equal(r.cQ.ewise("SUB", dec, dec0), m[:L1])
    assert np.array_equal(r.cQ.ewise("REDUCE", r.cQ.ewise("SUB", rec0, rec)), m)


def test_bfv_shares_cancel_the_mask(oracle, pkg):
    N, Q, P = _small(pkg, "bfv")
    r = ref.Refresh(oracle, N, Q, P, ref.BFV_T)
    rng = np.random.default_rng(8)
    sk, c1, crs = keygen_ref.uniform(rng, Q + P, N), keygen_ref.uniform(rng, Q, N), keygen_ref.uniform(rng, Q + P, N)
    e = ref.regular_bytes(rng, (2, N))
    mask = rng.integers(0, ref.BFV_T, N).astype(np.uint64)
    mask[:2] = [0, ref.BFV_T - 1]
    dec0, rec0 = r.bfv_gen_shares(sk, c1, crs, np.zeros(N, dtype=np.uint64), e[0], e[1])
    dec, rec = r.bfv_gen_shares(sk, c1, crs, mask, e[0], e[1])
    assert np.array_equal(r.cQ.ewise("ADD", dec, rec), r.cQ.ewise("ADD", dec0, rec0))
    assert np.array_equal(r.cQ.ewise("SUB", dec, dec0), r.lift(mask))


@pytest.mark.parametrize("name", ["n16", "PN13QP218"])
def test_recode_of_hand_set_integers(oracle, pkg, name):
    """v in {0, 1, (Q_ls - 1) / 2 - 1, (Q_ls - 1) / 2, (Q_ls + 1) / 2, Q_ls - 1} -> v mod q_i for every limb, centred from Q_ls >> 1 up;
    the copy of rows 0 .. levelStart and the Garner route give the same"""
    N = 1 << 4
    Q = list(pkg.params.Qi60()[:2]) if name == "n16" else list(pkg.params.ckks_moduli(name)[1])
    r = ref.Refresh(oracle, N, Q)
    for ls in range(len(Q)):
        Qls = ref.product(Q[:ls + 1])
        hand = [0, 1, (Qls - 1) // 2 - 1, (Qls - 1) // 2, (Qls + 1) // 2, Qls - 1, Qls >> 1, (Qls >> 1) - 1]
        rng = np.random.default_rng(ls)
        v = (hand + [int.from_bytes(rng.bytes(8 * len(Q)), "little") % Qls for _ in range(N)])[:N]
        p_in = r.cQ.ntt(np.array([[x % q for x in v] for q in Q[:ls + 1]], dtype=np.uint64))
        centred = [x - Qls if x >= Qls >> 1 else x for x in v]
        assert centred[3] == (Qls - 1) // 2 - Qls and centred[2] == (Qls - 1) // 2 - 1          # Q_ls is odd: Q_ls >> 1 = (Q_ls - 1) / 2
        want = r.cQ.ntt(np.array([[x % q for x in centred] for q in Q], dtype=np.uint64))
        assert np.array_equal(r.ckks_recode(p_in), want), ls
        assert np.array_equal(r.ckks_recode_default(p_in), want), ls
        coeff = r.cQ.intt(p_in)
        for j in range(N):
            assert ref.garner_recode(Q, ls, coeff[:, j]) == [centred[j] % q for q in Q], (ls, j)


@pytest.mark.parametrize("level_start", [0, 1])
def test_default_ckks_shapes_give_the_restatements_bits(oracle, pkg, level_start):
    N, Q, _ = _small(pkg, "ckks")
    r = ref.Refresh(oracle, N, Q)
    sk, c1, crs, e = _ckks_case(oracle, pkg, N, Q)
    masks, _ = _edge_masks(Q, level_start, N)
    a, b = r.ckks_gen_shares(level_start, sk, c1, crs, masks, e[0], e[1]), r.ckks_gen_shares_default(level_start, sk, c1, crs, masks, e[0], e[1])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    c0 = keygen_ref.uniform(np.random.default_rng(3), Q, N)
    assert np.array_equal(r.ckks_finalize(level_start, c0, a[0], a[1]), r.ckks_finalize(level_start, c0, a[0], a[1], recode=r.ckks_recode_default))


def test_default_bfv_shape_gives_the_restatements_bits(oracle, pkg):
    """hP written as 0 where (magnitude 0, sign 0) leaves p_j: no bit of either share changes"""
    N, Q, P = _small(pkg, "bfv")
    r = ref.Refresh(oracle, N, Q, P, ref.BFV_T)
    rng = np.random.default_rng(9)
    sk, c1, crs = keygen_ref.uniform(rng, Q + P, N), keygen_ref.uniform(rng, Q, N), keygen_ref.uniform(rng, Q + P, N)
    e = ref.regular_bytes(rng, (2, N))
    e[0, :8] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80, 0, 0]
    e[0, N - 1] = 0
    mask = rng.integers(0, ref.BFV_T, N).astype(np.uint64)
    a, b = r.bfv_gen_shares(sk, c1, crs, mask, e[0], e[1]), r.bfv_gen_shares(sk, c1, crs, mask, e[0], e[1], hp_zero=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.fixture(scope="module")
def params(pkg):
    N, Q, P = pkg.params.ckks_moduli(ref.REFRESH_PARAMS)
    return N, list(Q), list(P)


def test_three_party_ckks_chains(oracle, pkg, params):
    """levelStart 0 and 1, seeds 0 .. 2: the refreshed ciphertext is at level L and decodes within REFRESH_TOLERANCE"""
    import ckks_encoder_ref
    N, Q, P = params
    roots = ckks_encoder_ref.roots_table(N)
    worst = 0.0
    for level_start in (0, 1):
        for seed in range(3):
            w = ref.oracle_refresh(oracle, "ckks", N, Q, P, seed, level_start, roots)
            assert w["out"].shape == (2, len(Q), N)
            err = float(np.max(np.abs(w["decoded"] - w["values"])))
            print("refresh levelStart %d seed %d: largest slot error %.6e" % (level_start, seed, err))
            worst = max(worst, err)
    print("largest slot error %.6e (REFRESH_MEASURED %.6e, allowed %.6e)" % (worst, ref.REFRESH_MEASURED, ref.REFRESH_TOLERANCE))
    assert worst <= ref.REFRESH_TOLERANCE


def test_three_party_bfv_chain(oracle, pkg):
    """t = 65537: the ciphertext of a ciphertext x plaintext product is refreshed, decrypts to the same plaintext exactly, with less
    noise than before"""
    N, Q, P, _ = pkg.params.bfv_moduli(ref.REFRESH_PARAMS)
    w = ref.oracle_refresh(oracle, "bfv", N, list(Q), list(P), 0)
    assert np.array_equal(w["decoded"], w["expected"])
    before = ref.bfv_noise(w["ref"], w["ct"], w["sk"], w["expected_poly"])
    after = ref.bfv_noise(w["ref"], w["out"], w["sk"], w["expected_poly"])
    print("noise: %d bits before the refresh, %d bits after" % (before.bit_length(), after.bit_length()))
    assert after < before
