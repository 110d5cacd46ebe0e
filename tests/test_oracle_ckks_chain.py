"""tests/ckks_chain_ref.py pinned on the CPU, independently of the device code: its step lists against the reference's index tables
(ring.PermuteNTTIndex(GaloisGen, +-2^i, N), ckks/keygen.go:407-408), and the chain itself on a key-free stand-in -- key images of zeros, so
that switchKeysInPlace returns (0, 0) and a step is (PermuteNTT(a0), 0): the chain over the bits of k permutes like the single element 5^k,
and the accumulating chain follows a <- PermuteNTT(a) + a, checked against Python integers."""
import numpy as np
import pytest

import ckks_chain_ref as chain_ref

N = 1 << 5


@pytest.fixture(scope="module")
def small(oracle, pkg):
    _, Q, P = pkg.params.ckks_moduli("PN12QP109")
    Q, P = [int(q) for q in Q[:2]], [int(p) for p in P[:1]]
    cQ = oracle.Context(N, Q)
    oplan = oracle.CkksPlan(cQ, oracle.Context(N, P))
    rng = np.random.default_rng(7)
    ct = np.stack([np.stack([rng.integers(0, q, N, dtype=np.uint64) for q in Q]) for _ in range(2)])
    ct[0, :, 3] = 0
    ct[1, :, 5] = np.array(Q, dtype=np.uint64) - 1
    zero_key = np.zeros((len(Q), 2, len(Q) + len(P), N), dtype=np.uint64)       # beta = |Q| / |P| = 2
    return dict(Q=Q, cQ=cQ, oplan=oplan, ct=ct, key=zero_key)


def test_step_lists_are_the_reference_index_tables(small):
    cQ = small["cQ"]
    assert chain_ref.pow2_steps(N, 5) == [(5, 1), (pow(5, 4, 2 * N), 4)]
    assert chain_ref.pow2_steps(N, 6, left=False) == [(pow(5, -2, 2 * N), 2), (pow(5, -4, 2 * N), 4)]
    assert chain_ref.slot_sum_elements(N) == [pow(5, 1 << i, 2 * N) for i in range(4)]
    for left in (True, False):
        for g, idx in chain_ref.pow2_steps(N, (N >> 1) - 1, left):
            table = cQ.permute_ntt_index(5, idx if left else 2 * N - idx)      # permuteNTTLeftIndex[2^i] / permuteNTTRightIndex[2^i]
            assert np.array_equal(cQ.permute_ntt_index(g, 1), table), (left, idx)


@pytest.mark.parametrize("k,left", [(5, True), ((N >> 1) - 1, True), (6, False)])
def test_replace_chain_permutes_like_the_single_element(small, k, left):
    s = small
    level = len(s["Q"]) - 1
    out = chain_ref.rotate_columns_pow2(s["oplan"], level, N, s["Q"], s["ct"], k, {1 << i: s["key"] for i in range(4)}, left)
    g = pow(5, k if left else -k, 2 * N)
    assert np.array_equal(out[0], s["cQ"].permute_ntt(s["ct"][0], g))
    assert not out[1].any()                                                     # p1 of a zero key


def test_accumulating_chain_follows_its_recursion(small):
    s = small
    Q, level = s["Q"], len(s["Q"]) - 1
    gens = chain_ref.slot_sum_elements(N)
    out = chain_ref.chain(s["oplan"], level, Q, s["ct"], gens, [s["key"]] * len(gens), True)
    a = [[int(x) for x in row] for row in s["ct"][0]]
    for g in gens:
        index = [int(i) for i in s["cQ"].permute_ntt_index(g, 1)]
        a = [[(row[index[j]] + row[j]) % q for j in range(N)] for row, q in zip(a, Q)]
    assert out[0].tolist() == a
    assert np.array_equal(out[1], s["ct"][1])                                   # 0 + a1 at every step
