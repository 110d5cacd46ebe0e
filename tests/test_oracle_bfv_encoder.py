"""The restatement of bfv.Encoder (tests/bfv_encoder_ref.py) means what the BFV batch encoding says, at N <= 2^6 with Python integers as the
arbiter: indexMatrix is a permutation, deltaMont is floor(Q / t) in Montgomery form, encode followed by decode is the identity for every
plaintext modulus the device tests use, partially filled slot vectors decode with a zero tail, the lift equals floor(Q / t) m modulo every
q_i, and the negacyclic product of two encodings decodes to the slot-wise product.  CPU only."""
import numpy as np
import pytest

import bfv_encoder_ref as ref

T40 = 1099512938497          # GenerateNTTPrimes(40, 16, 1)[0] = 2^40 + 10 * 2^17 + 1
MODULI_T = [17, 12289, 40961, 65537, 786433, 0x3ee0001, 2013265921, T40]


def _Q(pkg, limbs=2):
    return list(pkg.params.Qi60()[:limbs])


def _sizes(t):
    return [N for N in (8, 16, 64) if (t - 1) % (2 * N) == 0]


def _slots(t, n, seed, signed=False):
    rng = np.random.default_rng(seed)
    if signed:
        return rng.integers(-(t // 2), t // 2 + 1, size=n, dtype=np.int64)
    return rng.integers(0, t, size=n, dtype=np.uint64)


def test_the_forty_bit_modulus_is_the_generated_prime(pkg):
    assert pkg.params.GenerateNTTPrimes(40, 16, 1)[0] == T40 and pkg.params.is_prime(T40)


@pytest.mark.parametrize("N", [2, 8, 64, 1 << 12])
def test_index_matrix_is_a_permutation(N):
    assert sorted(int(x) for x in ref.index_matrix(N)) == list(range(N))


def test_delta_mont_is_floor_q_over_t(oracle, pkg):
    Q = _Q(pkg, 3)
    big = Q[0] * Q[1] * Q[2]
    for t in (17, 65537, T40):
        dm = ref.delta_mont(oracle, Q, t)
        assert [oracle.inv_mform(int(d), q) for d, q in zip(dm, Q)] == [(big // t) % q for q in Q]


@pytest.mark.parametrize("t", MODULI_T)
def test_round_trip_and_zero_tail(oracle, pkg, t):
    sizes = _sizes(t)
    assert sizes
    for N in sizes:
        enc = ref.Encoder(oracle, N, _Q(pkg), t)
        for n in sorted({0, 1, N // 2 + 1, N}):
            u = _slots(t, n, 3 * N + n)
            got = enc.decode_uint(enc.encode_uint(u))
            assert np.array_equal(got[:n], u) and not got[n:].any(), (N, n)
            s = _slots(t, n, 5 * N + n, signed=True)
            got = enc.decode_int(enc.encode_int(s))
            assert np.array_equal(got[:n], s) and not got[n:].any(), (N, n)


def test_values_outside_the_canonical_range(oracle, pkg):
    t, N = 65537, 16
    enc = ref.Encoder(oracle, N, _Q(pkg), t)
    u = np.array([t, t + 5, 2**64 - 1, 0, t - 1], dtype=np.uint64)
    assert [int(x) for x in enc.decode_uint(enc.encode_uint(u))[:5]] == [0, 5, (2**64 - 1) % t, 0, t - 1]
    s = np.array([-1, -(t - 1) // 2, t >> 1, (t >> 1) + 1, -t, -2**63], dtype=np.int64)
    assert [int(x) for x in enc.decode_int(enc.encode_int(s))[:6]] == [-1, -(t - 1) // 2, t >> 1, (t >> 1) + 1 - t, 0, ((-2**63) % t + t // 2) % t - t // 2]
    with pytest.raises(ValueError):
        enc.encode_uint(np.zeros(N + 1, dtype=np.uint64))


def test_the_lift_is_delta_times_the_message(oracle, pkg):
    """encodePlaintext's MRed(m[j], deltaMont[i], q_i) against Python integers and against the oracle's scalar MRed"""
    t, N = 12289, 8
    Q = _Q(pkg, 3)
    enc = ref.Encoder(oracle, N, Q, t)
    u = _slots(t, N, 11)
    pt = enc.encode_uint(u)
    m = enc.cT.intt(enc._scatter(u)[None])[0]
    delta = (Q[0] * Q[1] * Q[2]) // t
    for i, q in enumerate(Q):
        assert [int(x) for x in pt[i]] == [delta * int(x) % q for x in m]
        assert [int(x) for x in pt[i]] == [oracle.mred(int(x), int(enc.delta_mont[i]), q) for x in m]


@pytest.mark.parametrize("t,N", [(17, 8), (65537, 64), (T40, 16)])
def test_product_of_encodings_decodes_to_the_slot_wise_product(oracle, pkg, t, N):
    Q = _Q(pkg)
    enc = ref.Encoder(oracle, N, Q, t)
    a, b = _slots(t, N, 21), _slots(t, N, 22)
    ma = [int(x) for x in enc.cT.intt(enc._scatter(a)[None])[0]]
    mb = [int(x) for x in enc.cT.intt(enc._scatter(b)[None])[0]]
    prod = [0] * N
    for i in range(N):
        for j in range(N):
            k, sign = (i + j) % N, -1 if i + j >= N else 1
            prod[k] = (prod[k] + sign * ma[i] * mb[j]) % t
    delta = (Q[0] * Q[1]) // t
    pt = np.array([[delta * x % q for x in prod] for q in Q], dtype=np.uint64)
    assert [int(x) for x in enc.decode_uint(pt)] == [int(x) * int(y) % t for x, y in zip(a, b)]


def test_a_sixty_bit_t_is_parity_only(oracle, pkg):
    """a 60-bit t against a 120-bit Q: SimpleScaler's double-double fraction no longer carries the message, so encode / decode is NOT the
    identity there -- the device tests hold such a t to the restatement, not to the round trip"""
    N = 16
    t = pkg.params.Pi60()[0]
    enc = ref.Encoder(oracle, N, _Q(pkg), t)
    u = _slots(t, N, 31)
    pt = enc.encode_uint(u)
    assert pt.shape == (2, N)
    assert not np.array_equal(enc.decode_uint(pt), u)


def test_a_modulus_without_the_root_is_refused(oracle, pkg):
    with pytest.raises(ValueError):
        ref.Encoder(oracle, 64, _Q(pkg), 17)
