"""Test helper (not a test module): ckks.Encoder (ckks/encoder.go:31-226), scaleUpVecExact and scaleDown (ckks/utils.go:51-114) restated
line by line for one plaintext at a time.  The special FFTs work on a float64 array of real and one of imaginary parts, and every
butterfly is written as separate real operations (numpy's element-wise +, -, * on float64 are single IEEE operations, so nothing can be
fused and no complex product of numpy's is used); Python integers stand for big.Int and big.Float (float(int) rounds to nearest-even as
big.Float.SetInt(..).Float64() does).  The CPU oracle supplies NTTLvl / InvNTTLvl.  The root table is an input: Go's math.Cos / math.Sin
differ from libm in the last place, so parity needs the caller's table."""
import math

import numpy as np

GALOIS_GEN = 5
TWO64 = 1.8446744073709552e+19


def roots_table(N, cos=math.cos, sin=math.sin):
    """:47-53: roots[0 .. m] as a complex128 array, from the reference's expression for the angle"""
    m = 2 * N
    r = np.empty(m + 1, dtype=np.complex128)
    for i in range(m):
        angle = 2 * 3.141592653589793 * float(i) / float(m)
        r[i] = complex(cos(angle), sin(angle))
    r[m] = r[0]
    return r


def rot_group(N):
    """:39-45: m / 2 entries, the first m / 4 filled"""
    m = 2 * N
    g = np.zeros(m >> 1, dtype=np.uint64)
    five = 1
    for i in range(m >> 2):
        g[i] = five
        five = (five * GALOIS_GEN) & (m - 1)
    return g


def bit_reverse_perm(n):
    bits = n.bit_length() - 1
    return np.array([int(format(i, "0%db" % bits)[::-1], 2) if bits else 0 for i in range(n)], dtype=np.int64)


def scale_up_exact(x, scale, q):
    """one coefficient and one modulus of scaleUpVecExact (ckks/utils.go:51-98)"""
    x, scale, q = float(x), float(scale), int(q)
    y = scale * x
    if y > TWO64:
        # big.NewFloat(y) has 53 bits: Add(0.5) rounds back to y, Int() is the exact integer of the double
        r = int(y) % q
        return q - r if x < 0 else r
    if x < 0:
        return q - (int(-scale * x + 0.5) % q)
    return int(y + 0.5) % q


def centre(x, Q):
    """:138-142: x mod Q, minus Q from Q >> 1 up"""
    x %= Q
    return x - Q if x >= (Q >> 1) else x


def scale_down(x, scale):
    """ckks/utils.go:108-114: the exact integer to the nearest double (ties to even, +-Inf from 2^1024), then an IEEE division"""
    try:
        f = float(x)
    except OverflowError:
        f = math.inf if x > 0 else -math.inf
    return f / float(scale)


class Encoder:
    """ckks.NewEncoder for (N, Q); plaintexts are [level + 1, N] uint64 in the NTT domain"""

    def __init__(self, oracle, N, Q, roots=None):
        self.oracle, self.N, self.Q = oracle, int(N), [int(q) for q in Q]
        self.cQ = oracle.Context(N, self.Q) if oracle is not None else None
        self.m = 2 * self.N
        self.max_slots = self.N >> 1
        self.rot = rot_group(self.N)
        self.roots = roots_table(self.N) if roots is None else np.asarray(roots, dtype=np.complex128)
        self._rot_int = [int(v) for v in self.rot]

    def _stage_roots(self, length, inverse):
        lenh, lenq = length >> 1, length << 2
        gap = self.m // lenq
        if inverse:
            idx = [(lenq - (self._rot_int[j] % lenq)) * gap for j in range(lenh)]            # :181
        else:
            idx = [(self._rot_int[j] % lenq) * gap for j in range(lenh)]                     # :217
        w = self.roots[idx]
        return w.real.copy(), w.imag.copy()

    def invfft(self, values):
        """:170-202 on a complex128 vector of `slots` entries; returns (re, im) float64 arrays"""
        n = len(values)
        re, im = np.array(values.real, dtype=np.float64), np.array(values.imag, dtype=np.float64)
        length = n
        while length >= 2:
            lenh = length >> 1
            wr, wi = self._stage_roots(length, True)
            r, i = re.reshape(-1, length), im.reshape(-1, length)
            ar, ai, br, bi = r[:, :lenh].copy(), i[:, :lenh].copy(), r[:, lenh:].copy(), i[:, lenh:].copy()
            vr, vi = ar - br, ai - bi
            r[:, :lenh], i[:, :lenh] = ar + br, ai + bi
            p0, p1, p2, p3 = vr * wr, vi * wi, vr * wi, vi * wr
            r[:, lenh:], i[:, lenh:] = p0 - p1, p2 + p3
            length >>= 1
        perm = bit_reverse_perm(n)
        re, im = re[perm], im[perm]
        # values[i] /= complex(float64(N), 0): Go's complex128div gives ((re + im * 0) / N, (im - re * 0) / N)
        nf = np.float64(n)
        return (re + im * 0.0) / nf, (im - re * 0.0) / nf

    def fft(self, re, im):
        """:204-226; returns a complex128 vector"""
        n = len(re)
        perm = bit_reverse_perm(n)
        re, im = np.array(re, dtype=np.float64)[perm], np.array(im, dtype=np.float64)[perm]
        length = 2
        while length <= n:
            lenh = length >> 1
            wr, wi = self._stage_roots(length, False)
            r, i = re.reshape(-1, length), im.reshape(-1, length)
            ur, ui, br, bi = r[:, :lenh].copy(), i[:, :lenh].copy(), r[:, lenh:].copy(), i[:, lenh:].copy()
            p0, p1, p2, p3 = br * wr, bi * wi, br * wi, bi * wr
            vr, vi = p0 - p1, p2 + p3
            r[:, :lenh], i[:, :lenh] = ur + vr, ui + vi
            r[:, lenh:], i[:, lenh:] = ur - vr, ui - vi
            length <<= 1
        out = np.empty(n, dtype=np.complex128)
        out.real, out.imag = re, im
        return out

    def coefficients(self, values):
        """:92-103: the N float64 coefficients Encode hands to scaleUpVecExact"""
        values = np.asarray(values, dtype=np.complex128)
        slots = len(values)
        assert slots >= 1 and slots & (slots - 1) == 0 and slots <= self.max_slots
        re, im = self.invfft(values)
        gap = self.max_slots // slots
        vf = np.zeros(self.N, dtype=np.float64)
        vf[0:self.max_slots:gap] = re
        vf[self.max_slots::gap] = im
        return vf

    def encode_coeffs(self, values, level, scale):
        """Encode up to scaleUpVecExact (:105): [level + 1, N] in the coefficient domain"""
        vf = self.coefficients(values)
        pt = np.zeros((level + 1, self.N), dtype=np.uint64)
        for c in np.nonzero(vf)[0]:
            for j in range(level + 1):
                pt[j, c] = scale_up_exact(vf[c], scale, self.Q[j])
        return pt

    def encode(self, values, level, scale):
        """:78-116"""
        return self.cQ.ntt(self.encode_coeffs(values, level, scale), level)

    def decode_coeffs(self, coeffs, slots, level, scale):
        """:122-154 from the coefficient-domain image [level + 1, N]"""
        Ql = 1
        for q in self.Q[:level + 1]:
            Ql *= q
        hats = [Ql // q for q in self.Q[:level + 1]]
        invs = [pow(h % q, -1, q) for h, q in zip(hats, self.Q[:level + 1])]
        gap = self.max_slots // slots

        def value(c):
            x = sum((int(coeffs[j, c]) * invs[j] % self.Q[j]) * hats[j] for j in range(level + 1))     # PolyToBigint, then Mod(Q_level)
            return scale_down(centre(x, Ql), scale)
        re = np.array([value(i * gap) for i in range(slots)], dtype=np.float64)
        im = np.array([value(self.max_slots + i * gap) for i in range(slots)], dtype=np.float64)
        return self.fft(re, im)

    def decode(self, pt, slots, level, scale):
        """:119-168"""
        pt = np.ascontiguousarray(np.asarray(pt, dtype=np.uint64)[:level + 1])
        return self.decode_coeffs(self.cQ.intt(pt, level), slots, level, scale)
