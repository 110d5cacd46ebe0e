"""tests/bfv_chain_ref.py pinned on the CPU, independently of the device code: on a small ring with real keys from the restated key
generator, the helper's InnerSum of an encrypted slot vector decrypts to the sum of the slots in every slot, and its replace chain
(rotateColumnsPow2, k = 5) to the slots rotated by 5 within each row.  A wrong Galois element or key order decrypts to noise."""
import numpy as np
import pytest

import bfv_chain_ref as chain_ref
import bfv_encoder_ref as encoder_ref
import bfv_encryptor_ref as encryptor_ref
import keygen_ref

N, T = 1 << 5, 65537      # t = 1 mod 2N: NTT-friendly


@pytest.fixture(scope="module")
def small(oracle, pkg):
    _, Q, P, _ = pkg.params.bfv_moduli("PN12QP109")      # 2 + 1 limbs
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    rng = np.random.default_rng(2024)
    kg = keygen_ref.KeyGenerator(oracle, N, Q, P, "bfv")
    sk = kg.gen_secret_key(keygen_ref.draw(rng, (N >> 3,)), keygen_ref.draw(rng, (N >> 3,)))
    rows = len(Q) + len(P)

    def rot_key(gen):
        key = kg.gen_rot_key(sk, gen, keygen_ref.draw(rng, shape_noise=(kg.beta, N)), keygen_ref.uniform(rng, Q + P, N, kg.beta))
        return key.reshape(kg.beta, 2, rows, N)
    left = {1 << i: rot_key(pow(5, 1 << i, 2 * N)) for i in range(4)}            # evakeyRotColLeft[2^i], bfv/keygen.go:381
    row = rot_key(2 * N - 1)                                                     # evakeyRotRow, :385
    coder = encoder_ref.Encoder(oracle, N, Q, T)
    values = rng.integers(0, T, N).astype(np.uint64)
    crp = keygen_ref.uniform(rng, Q, N)
    ct = encryptor_ref.Encryptor(oracle, N, Q, P).encrypt_sk(True, sk, crp, keygen_ref.draw(rng, shape_noise=(N,)), coder.encode_uint(values))
    cQ = oracle.Context(N, Q)
    oplan = oracle.CkksPlan(cQ, oracle.Context(N, P))
    slots = lambda c: coder.decode_uint(encryptor_ref.decrypt(cQ, c, sk))
    assert np.array_equal(slots(ct), values)
    return dict(Q=Q, oplan=oplan, ct=ct, values=values, left=left, row=row, slots=slots)


def test_inner_sum_of_the_helper_decrypts_to_the_sum_in_every_slot(small):
    s = small
    assert chain_ref.inner_sum_elements(N) == [5, 25, pow(5, 4, 64), pow(5, 8, 64), 63]
    out = chain_ref.inner_sum(s["oplan"], N, s["Q"], s["ct"], [s["left"][1 << i] for i in range(4)], s["row"])
    assert np.array_equal(s["slots"](out), np.full(N, int(s["values"].astype(object).sum()) % T, dtype=np.uint64))


def test_replace_chain_of_the_helper_rotates_the_rows(small):
    s = small
    assert chain_ref.pow2_steps(N, 5, 5) == [(5, 1), (pow(5, 4, 64), 4)]
    out = chain_ref.rotate_columns_pow2(s["oplan"], N, s["Q"], s["ct"], 5, 5, s["left"])
    want = np.roll(s["values"].reshape(2, N >> 1), -5, axis=1).reshape(N)      # RotateColumns: k positions to the left, row by row
    assert np.array_equal(s["slots"](out), want)
