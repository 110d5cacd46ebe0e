"""Test helper (not a test module): bfv.Encoder (bfv/encoder.go:28-182) and GenLiftParams (bfv/utils.go:9-23) restated line by line over
the CPU oracle's ring primitives -- Context(N, [t]).intt / ntt for contextT, MRed / MForm, SimpleScaler -- for one plaintext at a time.
GaloisGen = 5 (bfv/bfv.go).  Python integers only where the reference uses big.Int."""
import numpy as np

GALOIS_GEN = 5


def bit_reverse(x, bits):
    r = 0
    for i in range(bits):
        r |= ((x >> i) & 1) << (bits - 1 - i)
    return r


def index_matrix(N):
    """bfv/encoder.go:36-58"""
    logN = N.bit_length() - 1
    row, m, pos = N >> 1, N << 1, 1
    index = [0] * N
    for i in range(row):
        index[i] = bit_reverse((pos - 1) >> 1, logN)
        index[i | row] = bit_reverse((m - pos - 1) >> 1, logN)
        pos = (pos * GALOIS_GEN) & (m - 1)
    return np.array(index, dtype=np.uint64)


def delta_mont(oracle, Q, t):
    """GenLiftParams: MForm(floor(Q / t) mod q_i)"""
    big = 1
    for q in Q:
        big *= int(q)
    delta = big // int(t)
    return np.array([oracle.mform(delta % int(q), int(q)) for q in Q], dtype=np.uint64)


class Encoder:
    """bfv.NewEncoder(params) for (N, Q, t); plaintexts are [|Q|, N] uint64 over Q in the coefficient domain"""

    def __init__(self, oracle, N, Q, t):
        self.oracle, self.N, self.Q, self.t = oracle, int(N), [int(q) for q in Q], int(t)
        self.cQ = oracle.Context(N, self.Q)
        self.cT = oracle.Context(N, [self.t])              # raises where the reference returns "does not allow NTT"
        self.index = index_matrix(self.N)
        self.delta_mont = delta_mont(oracle, self.Q, self.t)
        self.scaler = oracle.SimpleScaler(self.t, self.cQ)

    # :121-137: InvNTT over contextT, then limb i = MRed(m[j], deltaMont[i], q_i) (MulCoeffsMontgomery is that loop over all limbs)
    def _encode_plaintext(self, row):
        m = self.cT.intt(row[None])[0]
        lifted = np.broadcast_to(m, (len(self.Q), self.N)).copy()
        delta = np.broadcast_to(self.delta_mont[:, None], (len(self.Q), self.N)).copy()
        return self.cQ.ewise("MUL_MONT", lifted, delta)

    def _scatter(self, residues):
        if len(residues) > self.N:
            raise ValueError("invalid input to encode (number of coefficients must be smaller or equal to the context)")      # :73, :97
        row = np.zeros(self.N, dtype=np.uint64)
        row[self.index[:len(residues)].astype(np.int64)] = residues
        return row

    def encode_uint(self, values):
        """:71-91, the values taken modulo t"""
        v = np.asarray(values, dtype=np.uint64)
        return self._encode_plaintext(self._scatter(v % np.uint64(self.t)))

    def encode_int(self, values):
        """:95-119: t + c for a negative c; here the residue in [0, t) of any int64 (the same for -t <= c < t)"""
        v = np.array([int(x) % self.t for x in np.asarray(values, dtype=np.int64)], dtype=np.uint64)
        return self._encode_plaintext(self._scatter(v))

    def _decode(self, pt):
        pool = self.scaler.scale(np.ascontiguousarray(pt, dtype=np.uint64), limbs_out=1)       # :142
        pool = self.cT.ntt(pool)                                                               # :144
        return pool[0][self.index.astype(np.int64)]                                            # :148-150

    def decode_uint(self, pt):
        return self._decode(pt)

    def decode_int(self, pt):
        """:158-182"""
        v = self._decode(pt).astype(np.int64)
        return np.where(v > (self.t >> 1), v - self.t, v)
