"""Test helper (not a test module): pkEncryptor.encrypt (bfv/encryptor.go:169-223), skEncryptor.encrypt (:306-345) and decryptor.Decrypt
(bfv/decryptor.go:55-75) restated line by line over the CPU oracle's ring primitives -- Context.ntt / intt / ewise and
BasisExtender.moddown_pq -- for one ciphertext at a time, after the sampling: the samplers' decisions arrive in compact form (the two bit
planes of sampleTernary at p = 0.5, one (magnitude, sign) byte per Gaussian coefficient) and are expanded here with plain numpy and
Python integers.  Polys are [limbs, N] uint64; polys over Q||P hold contextQP's limbs, Q first."""
import numpy as np


def expand_ternary(oracle, moduli, coeff_bits, sign_bits, N):
    """sampleTernary at p = 0.5 (ring/ternarySampler.go:157-177) with samplerMatrix = matrixTernaryMontgomery
    (ring/ring_context.go:119-122): [0, MForm(1), MForm(q - 1)] per modulus"""
    coeff_bits, sign_bits = np.asarray(coeff_bits, dtype=np.uint8), np.asarray(sign_bits, dtype=np.uint8)
    assert coeff_bits.shape == sign_bits.shape == (N >> 3,)
    matrix = [[0, oracle.mform(1, int(q)), oracle.mform(int(q) - 1, int(q))] for q in moduli]
    i = np.arange(N)
    coeff = (coeff_bits[i >> 3].astype(np.int64) >> (i & 7)) & 1                 # :169
    sign = (sign_bits[i >> 3].astype(np.int64) >> (i & 7)) & 1                   # :170
    index = (coeff & (sign ^ 1)) | ((sign & coeff) << 1)                         # :172
    return np.stack([np.array(row, dtype=np.uint64)[index] for row in matrix])   # :175


def expand_gaussian(moduli, e_bytes, N):
    """KYSampler.Sample's store (ring/gaussianSampler.go:247) from (coeff | sign << 7): sign 1 -> coeff, sign 0 -> q - coeff"""
    e_bytes = np.asarray(e_bytes, dtype=np.uint8)
    assert e_bytes.shape == (N,)
    coeff, sign = (e_bytes & 127).astype(np.uint64), (e_bytes >> 7).astype(bool)
    return np.stack([np.where(sign, coeff, np.uint64(int(q)) - coeff) for q in moduli])


class Encryptor:
    """newEncryptor (bfv/encryptor.go:100-119) for (N, Q, P); P empty: no baseconverter, only the fast forms"""

    def __init__(self, oracle, N, Q, P):
        self.oracle, self.N = oracle, int(N)
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.cQ = oracle.Context(N, self.Q)
        self.cQP = oracle.Context(N, self.Q + self.P) if self.P else None
        self.baseconverter = oracle.BasisExtender(self.cQ, oracle.Context(N, self.P)) if self.P else None

    def _ring(self, fast):
        if fast:
            return self.cQ, self.Q
        if self.baseconverter is None:
            raise ValueError("modulus P is empty -> use instead the fast form")               # :123-125
        return self.cQP, self.Q + self.P

    def encrypt_pk(self, fast, pk0, pk1, coeff_bits, sign_bits, e0, e1, pt):
        """:169-223.  In the fast branch the reference leaves polypool[0], polypool[1] in its pool and never writes them to the
        ciphertext (v1.3.1); the restatement, like the device, returns them as the ciphertext."""
        ctx, moduli = self._ring(fast)
        L = len(moduli)
        pool2 = ctx.ntt(expand_ternary(self.oracle, moduli, coeff_bits, sign_bits, self.N))    # :176 / :196 SampleTernaryMontgomeryNTT
        pool0 = ctx.ewise("MUL_MONT", pool2, np.asarray(pk0)[:L])                              # :178 / :200
        pool1 = ctx.ewise("MUL_MONT", pool2, np.asarray(pk1)[:L])                              # :179 / :201
        pool0, pool1 = ctx.intt(pool0), ctx.intt(pool1)                                        # :181-182 / :203-204
        pool0 = ctx.ewise("ADD", pool0, expand_gaussian(moduli, e0, self.N))                   # :185-186 / :207-208
        pool1 = ctx.ewise("ADD", pool1, expand_gaussian(moduli, e1, self.N))                   # :189-190 / :211-212
        if fast:
            c0, c1 = pool0, pool1
        else:
            level = len(self.Q) - 1
            c0 = self.baseconverter.moddown_pq(level, pool0)                                   # :215
            c1 = self.baseconverter.moddown_pq(level, pool1)                                   # :216
        return np.stack([self.cQ.ewise("ADD", c0, pt), c1])                                    # :222

    def encrypt_sk(self, fast, sk, crp, e, pt):
        """:306-345; crp = the uniform poly in the NTT domain (the reference works on its copy in polypool[1], :296-304)"""
        ctx, moduli = self._ring(fast)
        L = len(moduli)
        crp = np.asarray(crp, dtype=np.uint64)[:L]
        pool0 = ctx.ewise("MUL_MONT", crp, np.asarray(sk)[:L])                                 # :314 / :326
        pool0 = ctx.ewise("NEG", pool0)                                                        # :315 / :327 (q - x: a zero product gives q)
        pool0 = ctx.intt(pool0)                                                                # :317 / :330
        pool1 = ctx.intt(crp)                                                                  # :318 / :331
        pool0 = ctx.ewise("ADD", pool0, expand_gaussian(moduli, e, self.N))                    # :320 / :333 CRed(x + residue)
        if not fast:
            level = len(self.Q) - 1
            pool0 = self.baseconverter.moddown_pq(level, pool0)                                # :335
            pool1 = self.baseconverter.moddown_pq(level, pool1)                                # :336
        return np.stack([self.cQ.ewise("ADD", pool0, pt), pool1])                              # :344


def decrypt(cQ, ct, sk):
    """decryptor.Decrypt (bfv/decryptor.go:55-75); ct = [degree + 1, |Q|, N] in the coefficient domain, sk in NTT + Montgomery form (its
    first |Q| limbs are read)"""
    ct = np.asarray(ct, dtype=np.uint64)
    degree, L = ct.shape[0] - 1, cQ.L
    sk = np.asarray(sk, dtype=np.uint64)[:L]
    pt = cQ.ntt(ct[degree])                                                                    # :58
    for i in range(degree, 0, -1):
        pt = cQ.ewise("MUL_MONT", pt, sk)                                                      # :61
        pool = cQ.ntt(ct[i - 1])                                                               # :62
        pt = cQ.ewise("ADD", pt, pool)                                                         # :63
        if i & 7 == 7:
            pt = cQ.ewise("REDUCE", pt)                                                        # :66
    if degree & 7 != 7:
        pt = cQ.ewise("REDUCE", pt)                                                            # :71
    return cQ.intt(pt)                                                                         # :74


def keygen(oracle, N, moduli, rng):
    """bfv/keygen.go:92-133 over contextQP = (N, moduli): sk ternary in Montgomery + NTT form, pk = (-(s a + e), a) in the NTT domain;
    the samplers' decisions come from `rng` (a numpy Generator).  Returns (sk, pk0, pk1) and the ternary secret as a list of -1 / 0 / 1."""
    ctx = oracle.Context(N, moduli)
    s = [int(v) for v in rng.integers(-1, 2, N)]
    mont = [{0: 0, 1: oracle.mform(1, int(q)), -1: oracle.mform(int(q) - 1, int(q))} for q in moduli]
    sk = np.array([[m[v] for v in s] for m in mont], dtype=np.uint64)
    sk = ctx.ntt(sk)                                                                           # :94 SampleTernaryMontgomeryNTTNew
    e_bytes = (rng.integers(0, 20, N) | (rng.integers(0, 2, N) << 7)).astype(np.uint8)
    pk0 = ctx.ntt(expand_gaussian(moduli, e_bytes, N))                                         # :129 SampleNTTNew
    pk1 = np.array([rng.integers(0, int(q), N, dtype=np.uint64) for q in moduli], dtype=np.uint64)   # :130 NewUniformPoly
    pk0 = ctx.ewise("MUL_MONT_AND_ADD", sk, pk1, out=pk0)                                      # :132
    pk0 = ctx.ewise("NEG", pk0)                                                                # :133
    return sk, pk0, pk1, s
