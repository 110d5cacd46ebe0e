"""The restatement of ckks.Encoder (tests/ckks_encoder_ref.py) means what the CKKS encoding says, pinned independently of its own FFTs:
slot i of Decode(p) is p(zeta^(5^i mod 2N)) / scale evaluated directly from the integer coefficients, for every power-of-two slot count;
Decode(Encode(v)) is within N / scale of v; scaleUpVecExact's branches against exact rationals and Python integers around 2^52, 2^63 and
2^64 and for negatives with a zero remainder; the integer-to-double step at rounding ties and the centring at Q >> 1.  CPU only."""
import cmath
import math
from fractions import Fraction

import numpy as np
import pytest

import ckks_encoder_ref as ref

SCALE = float(1 << 30)


def _Q(pkg, limbs=2):
    return list(pkg.params.Qi60()[:limbs])


def _slot_counts(N):
    return [1 << k for k in range(0, N.bit_length() - 1)]          # 1 .. N / 2


def _residues(coeffs, Q):
    return np.array([[int(c) % q for c in coeffs] for q in Q], dtype=np.uint64)


def test_tables():
    for N in (2, 16, 128):
        m = 2 * N
        rot = ref.rot_group(N)
        assert len(rot) == m // 2 and [int(x) for x in rot[:m // 4]] == [pow(5, i, m) for i in range(m // 4)] and not rot[m // 4:].any()
        roots = ref.roots_table(N)
        assert len(roots) == m + 1 and roots[m] == roots[0] == 1
        assert max(abs(roots[i] - cmath.exp(2j * math.pi * i / m)) for i in range(m)) < 1e-15


@pytest.mark.parametrize("logn", [4, 5, 6, 7])
def test_decode_evaluates_the_polynomial_at_the_rotation_group(oracle, pkg, logn):
    N, Q = 1 << logn, _Q(pkg)
    enc = ref.Encoder(oracle, N, Q)
    zeta = lambda e: cmath.exp(2j * math.pi * (e % (2 * N)) / (2 * N))
    for slots in _slot_counts(N):
        gap = (N // 2) // slots
        rng = np.random.default_rng(100 * logn + slots)
        coeffs = [0] * N
        for k in list(range(0, N // 2, gap)) + list(range(N // 2, N, gap)):
            coeffs[k] = int(rng.integers(-(1 << 20), (1 << 20) + 1))
        pt = oracle.Context(N, Q).ntt(_residues(coeffs, Q))
        got = enc.decode(pt, slots, len(Q) - 1, SCALE)
        S = sum(abs(c) for c in coeffs) / SCALE
        for i in range(slots):
            e = pow(5, i, 2 * N)
            want = sum(c * zeta(e * k) for k, c in enumerate(coeffs) if c) / SCALE
            # log2(slots) <= 6 butterfly stages and at most N terms of the direct sum, each rounded at 2^-53 of a magnitude <= S
            assert abs(got[i] - want) <= 1e-12 * max(S, 1e-300), (slots, i)


@pytest.mark.parametrize("logn", [4, 5, 6, 7])
def test_round_trip_within_n_over_scale(oracle, pkg, logn):
    N, Q = 1 << logn, _Q(pkg)
    enc = ref.Encoder(oracle, N, Q)
    for slots in _slot_counts(N):
        rng = np.random.default_rng(7 * logn + slots)
        ang, rad = rng.uniform(0, 2 * math.pi, slots), rng.uniform(0, 1, slots)
        v = rad * np.exp(1j * ang)                                                     # |v| <= 1
        for level in (0, 1):
            back = enc.decode(enc.encode(v, level, SCALE), slots, level, SCALE)
            assert np.max(np.abs(back - v)) <= N / SCALE, (slots, level)


def _independent_scale_up(x, scale, q):
    """scaleUpVecExact on exact rationals: the double product, then either the exact integer of it (above 2^64) or the + 0.5 rounded to a
    double (Fraction -> float is correctly rounded) and truncated"""
    y = float(scale) * float(x)                    # one IEEE product, as n * values[i]
    if y > 2.0 ** 64:
        num, den = Fraction(y).numerator, Fraction(y).denominator
        assert den == 1
        return num % q
    mag = Fraction(abs(y)) + Fraction(1, 2)
    w = math.floor(Fraction(float(mag)))
    return q - (w % q) if x < 0 else w % q


def test_scale_up_branches_against_python_integers(pkg):
    Q = _Q(pkg, 2) + [pkg.params.ckks_moduli("PN12QP109")[1][1]]
    cases = []
    for scale in (2.0 ** 30, 2.0 ** 40, 2.0 ** 55):
        for target in (2.0 ** 52, 2.0 ** 53, 2.0 ** 63, 2.0 ** 64):
            base = target / scale
            for x in (math.nextafter(base, 0), base, math.nextafter(base, math.inf), base * (1 - 2.0 ** -30), base * 1.5, base * 2 ** 20, base * 2 ** 300):
                cases.append((x, scale))
                if scale * x < 2.0 ** 63:
                    cases.append((-x, scale))
        cases += [(0.25 / scale, scale), (0.5 / scale, scale), (0.75 / scale, scale), (-0.5 / scale, scale), (-0.25 / scale, scale), (0.0, scale), (-0.0, scale)]
    hit_big = hit_small = 0
    for x, scale in cases:
        if scale * x == 2.0 ** 64 or not math.isfinite(scale * x):     # outside the reference's defined domain
            continue
        hit_big += scale * x > 2.0 ** 64
        hit_small += scale * x <= 2.0 ** 64
        for q in Q:
            assert ref.scale_up_exact(x, scale, q) == _independent_scale_up(x, scale, q), (x, scale, q)
    assert hit_big >= 9 and hit_small >= 40
    # a negative coefficient whose magnitude is a multiple of q gives q, not 0, as the reference does
    for q in Q:
        for k in (1, 2, 5):
            if k * q < 2 ** 53:
                assert ref.scale_up_exact(-float(k * q), 1.0, q) == q and ref.scale_up_exact(float(k * q), 1.0, q) == 0
        x = -float(q >> 10 << 10) / 2.0 ** 40                            # scale * x is an exact integer, congruent to -(q mod 2^10)
        assert ref.scale_up_exact(x, 2.0 ** 40, q) == q - ((q >> 10 << 10) % q)
    assert ref.scale_up_exact(-4.0, 2.0 ** 30, 1 << 31) == 1 << 31


def _nearest_even_double(x):
    """the integer x >= 0 rounded to 53 bits, ties to even, in integers; returns the rounded integer"""
    n = x.bit_length()
    if n <= 53:
        return x
    s = n - 53
    mant, rest, half = x >> s, x & ((1 << s) - 1), 1 << (s - 1)
    if rest > half or (rest == half and mant & 1):
        mant += 1
    return mant << s


def test_integer_to_double_at_ties_and_centring_boundaries(pkg):
    for k in (53, 54, 60, 64, 65, 100, 127, 128, 500, 1000):
        tie = (1 << k) + (1 << (k - 53))                               # halfway between two doubles, even mantissa below
        odd = (1 << k) + 3 * (1 << (k - 53))                           # halfway, odd mantissa below: rounds up
        for x in (tie - 1, tie, tie + 1, odd - 1, odd, odd + 1, (1 << (k + 1)) - 1, (1 << k) - 1):
            for s in (1, -1):
                got = ref.scale_down(s * x, 1.0)
                assert got == s * float(_nearest_even_double(x)) and int(got) == s * _nearest_even_double(x), (k, x)
        assert ref.scale_down(tie, 2.0 ** 30) == float(1 << k) / 2.0 ** 30
    assert ref.scale_down(1 << 1024, 1.0) == math.inf and ref.scale_down(-(1 << 1024), 4.0) == -math.inf
    assert ref.scale_down((1 << 1024) - (1 << 970), 1.0) == math.inf                 # rounds up to 2^1024
    assert ref.scale_down((1 << 1024) - (1 << 970) - 1, 1.0) == float.fromhex("0x1.fffffffffffffp+1023")
    for limbs in (1, 2, 6):
        Q = 1
        for q in _Q(pkg, limbs):
            Q *= q
        half = Q >> 1
        assert ref.centre(half - 1, Q) == half - 1 and ref.centre(half, Q) == half - Q and ref.centre(half + 1, Q) == half + 1 - Q
        assert ref.centre(0, Q) == 0 and ref.centre(Q - 1, Q) == -1 and ref.centre(Q + 3, Q) == 3


def test_decode_coefficients_are_the_centred_crt_value(oracle, pkg):
    """decode with one slot reads coefficients 0 and N / 2 alone: the slot is (x0 + i x1) / scale for the centred values"""
    N, Q = 16, _Q(pkg, 3)
    enc = ref.Encoder(oracle, N, Q)
    big = Q[0] * Q[1] * Q[2]
    for x0, x1 in ((5, -7), ((big >> 1) - 1, big >> 1), (-(1 << 100) - (1 << 47), (1 << 150) + (1 << 97))):
        coeffs = [0] * N
        coeffs[0], coeffs[N // 2] = x0, x1
        got = enc.decode_coeffs(_residues(coeffs, Q), 1, 2, SCALE)[0]
        assert got.real == ref.scale_down(ref.centre(x0, big), SCALE) and got.imag == ref.scale_down(ref.centre(x1, big), SCALE)
