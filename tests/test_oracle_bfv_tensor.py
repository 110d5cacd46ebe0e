"""The restatement of bfv tensorAndRescale for every operand degree (tests/bfv_tensor_ref.py) is faithful: its degree-1 branches give the
oracle's bits (oc_bfv_mul / oc_bfv_square), and its general branch (bfv/evaluator.go:371-415) means what BFV says -- a ciphertext times a
plaintext and a degree-2 x degree-1 product decrypt to the products of the messages.  CPU only; Python integers decide."""
import numpy as np
import pytest

import bfv_tensor_ref as ref

T = 65537


def _plan(oracle, pkg, name, logn):
    _, Q, _, QMul = pkg.params.bfv_moduli(name)
    N = 1 << logn
    return oracle.BfvPlan(oracle.Context(N, list(Q)), oracle.Context(N, list(QMul)), T)


@pytest.mark.parametrize("name,logn", [("PN12QP109", 10), ("PN13QP218", 9)])
def test_degree_one_branches_match_the_oracle(oracle, pkg, name, logn):
    plan = _plan(oracle, pkg, name, logn)
    Q, N = plan.cQ.moduli, plan.cQ.N
    a = [ref.uniform(Q, N, 10 + k) for k in range(2)]
    b = [ref.uniform(Q, N, 20 + k) for k in range(2)]
    assert np.array_equal(ref.tensor_and_rescale(plan, a, b), plan.mul(np.stack(a), np.stack(b)))
    assert np.array_equal(ref.tensor_and_rescale(plan, a, a, square=True), plan.square(np.stack(a)))


def test_general_squaring_equals_the_product_of_two_copies(oracle, pkg):
    """2 x 2 (the one squaring of the reachable domain): :379-402 and :405-413 give the same canonical residues"""
    plan = _plan(oracle, pkg, "PN12QP109", 10)
    a = [ref.uniform(plan.cQ.moduli, plan.cQ.N, 30 + k) for k in range(3)]
    sq = ref.tensor_and_rescale(plan, a, a, square=True)
    assert sq.shape == (5, plan.cQ.L, plan.cQ.N)
    assert np.array_equal(sq, ref.tensor_and_rescale(plan, a, [x.copy() for x in a]))


def test_receiver_of_larger_degree_gets_zero_tails(oracle, pkg):
    """ctOut of degree above d0 + d1: the zeroed accumulators (:373-376) come out as zero polys (a case the device call leaves to the host)"""
    plan = _plan(oracle, pkg, "PN12QP109", 10)
    Q, N = plan.cQ.moduli, plan.cQ.N
    a, b = [ref.uniform(Q, N, 40), ref.uniform(Q, N, 41)], [ref.uniform(Q, N, 42)]
    out = ref.tensor_and_rescale(plan, a, b, out_degree=3)
    assert np.array_equal(out[:2], ref.tensor_and_rescale(plan, a, b))
    assert not out[2:].any()


def test_ciphertext_times_plaintext_decrypts_to_the_product(oracle, pkg):
    """Mul(ct, pt, out) with pt = floor(Q/t) * m (encodePlaintext), PN12QP109: decrypts to m0 * m mod (X^N + 1, t)"""
    plan = _plan(oracle, pkg, "PN12QP109", 12)
    ocQ, N = plan.cQ, plan.cQ.N
    s = ref.small(N, 1, 5)
    m0 = np.random.default_rng(6).integers(0, T, size=N)
    m = np.random.default_rng(7).integers(0, T, size=N)
    ct = ref.encrypt(ocQ, T, s, m0, 100)
    assert ref.decrypt(ocQ, T, ct, s) == [int(x) for x in m0]
    out = ref.tensor_and_rescale(plan, ct, [ref.encode(ocQ.moduli, T, m)])
    assert out.shape == (2, ocQ.L, N)
    assert ref.decrypt(ocQ, T, out, s) == ref.negacyclic(m0, m, T)
    # control: the plaintext without the scaling by floor(Q/t) does not decrypt to the product
    bad = ref.tensor_and_rescale(plan, ct, [ref.residues(m, ocQ.moduli)])
    assert ref.decrypt(ocQ, T, bad, s) != ref.negacyclic(m0, m, T)


def test_degree_two_times_degree_one_decrypts_to_the_triple_product(oracle, pkg):
    """(ct0 x ct1) x ct2 without relinearisation: the degree-3 result decrypts against (1, s, s^2, s^3) to m0 m1 m2.  PN13QP218's moduli
    at logN 11 (depth 2: the noise, about 2^68, does not fit under PN12QP109's Delta / 2)"""
    plan = _plan(oracle, pkg, "PN13QP218", 11)
    ocQ, N = plan.cQ, plan.cQ.N
    s = ref.small(N, 1, 15)
    ms = [np.random.default_rng(16 + k).integers(0, T, size=N) for k in range(3)]
    cts = [ref.encrypt(ocQ, T, s, ms[k], 200 + 10 * k) for k in range(3)]
    c2 = ref.tensor_and_rescale(plan, cts[0], cts[1])
    assert np.array_equal(c2, plan.mul(np.stack(cts[0]), np.stack(cts[1])))
    assert ref.decrypt(ocQ, T, c2, s) == ref.negacyclic(ms[0], ms[1], T)
    c3 = ref.tensor_and_rescale(plan, list(c2), cts[2])
    assert c3.shape == (4, ocQ.L, N)
    assert ref.decrypt(ocQ, T, c3, s) == ref.negacyclic(ref.negacyclic(ms[0], ms[1], T), ms[2], T)
