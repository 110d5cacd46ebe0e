"""tests/bfv_relin_ref.py pinned on the CPU, independently of the device code, on small rings (N = 16 and 64, 2 + 1 limbs): at degree 2 the
helper is the oracle's own bfv_relinearize bit for bit; at degree 3 on canonical inputs it is two successive degree-2 steps -- (ct[0],
ct[1], ct[3]) under the key from s^3, then (that, ct[2]) under the key from s^2 -- which pins the order of degrees and keys; and its CRed
is the single conditional subtraction, not a remainder."""
import numpy as np
import pytest

import bfv_relin_ref as relin_ref


@pytest.fixture(scope="module", params=[16, 64])
def small(request, oracle, pkg):
    N = request.param
    _, Q, P, _ = pkg.params.bfv_moduli("PN12QP109")      # 2 + 1 limbs
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    beta = -(-len(Q) // len(P))
    ct = pkg.sampling.uniform_poly(Q, N, 4, seed=500 + N).reshape(4, len(Q), N)
    keys = [pkg.sampling.uniform_poly(Q + P, N, 2 * beta, seed=510 + N + k).reshape(beta, 2, len(Q) + len(P), N) for k in range(2)]
    return dict(N=N, Q=Q, ct=ct, keys=keys, oplan=oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P)))


def test_degree_two_is_the_oracles_relinearize(small):
    s = small
    got = relin_ref.relinearize(s["oplan"], s["Q"], s["ct"][:3], s["keys"][:1])
    assert np.array_equal(got, s["oplan"].bfv_relinearize(s["ct"][:3], s["keys"][0]))


def test_degree_three_is_two_degree_two_steps(small):
    s = small
    ct, keys = s["ct"], s["keys"]
    got = relin_ref.relinearize(s["oplan"], s["Q"], ct, keys)
    first = s["oplan"].bfv_relinearize(np.stack([ct[0], ct[1], ct[3]]), keys[1])
    want = s["oplan"].bfv_relinearize(np.stack([first[0], first[1], ct[2]]), keys[0])
    assert np.array_equal(got, want)
    assert not np.array_equal(got, relin_ref.relinearize(s["oplan"], s["Q"], ct, keys[::-1]))


def test_cred_is_one_conditional_subtraction():
    q = np.uint64(97)
    x = np.array([0, 96, 97, 98, 193, 194, 2 * 97 + 96], dtype=np.uint64)
    assert relin_ref.cred(x, q).tolist() == [0, 96, 0, 1, 96, 97, 193]
