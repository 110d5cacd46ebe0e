"""Test helper (not a test module): pkEncryptor.encrypt (ckks/encryptor.go:179-237) and skEncryptor.encrypt (:318-362) restated line by
line over the CPU oracle's ring primitives -- Context.ntt / intt / ewise and BasisExtender.moddown_pq / moddown_ntt_pq -- for one
ciphertext at a time, after the sampling.  The samplers' decisions arrive in the compact form of the BFV encryptor and are expanded by
tests/bfv_encryptor_ref.py's rules.  Polys are [limbs, N] uint64; polys over Q||P hold contextQP's limbs, Q first; plaintext and
ciphertext are in the NTT domain over limbs 0 .. level.

Below the top level the reference does not run (its Context calls walk every modulus of contextQ).  The restatement says what the device
does there: the fast forms are the reference's lines restricted to limbs 0 .. level; the forms through P follow the lines literally --
everything before the ModDown over all of Q||P, ModDownPQ(level) reading its "P part" at rows level + 1 .. level + |P|
(ring_basis_extension.go:256), ModDownNTTPQ(level) reading it at rows |Q| .. (:177)."""
import numpy as np

from bfv_encryptor_ref import expand_gaussian, expand_ternary, keygen  # noqa: F401  (keygen: ckks/keygen.go has the same lines)

# The round trip Encode -> Encrypt -> Decrypt -> Decode of tests/test_oracle_ckks_encryptor.py (PN12QP109, all slots, scale 2^32, top
# level, seeds 0 .. 2 x the four forms): the largest slot error of the restatement over those twelve runs, measured on the CPU, and what
# the tests allow -- 16 x that, which covers the spread of ternary and Gaussian draws across seeds.
ROUND_TRIP_MEASURED = 5.192493e-05
ROUND_TRIP_TOLERANCE = 16 * ROUND_TRIP_MEASURED


class Encryptor:
    """newEncryptor (ckks/encryptor.go:100-119) for (N, Q, P); P empty: no baseconverter, only the fast forms"""

    def __init__(self, oracle, N, Q, P):
        self.oracle, self.N = oracle, int(N)
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.cQ = oracle.Context(N, self.Q)
        self.cQP = oracle.Context(N, self.Q + self.P) if self.P else None
        self.baseconverter = oracle.BasisExtender(self.cQ, oracle.Context(N, self.P)) if self.P else None

    def _through_p(self):
        if self.baseconverter is None:
            raise ValueError("modulus P is empty -> use instead the fast form")               # :139-142
        return self.cQP, self.Q + self.P

    def sample_ntt(self, e_bytes, level):
        """gaussianSampler.SampleNTT: Sample, then Context.NTT"""
        return self.cQ.ntt(expand_gaussian(self.Q[:level + 1], e_bytes, self.N), level)

    def encrypt_pk(self, fast, level, pk0, pk1, coeff_bits, sign_bits, e0, e1, pt):
        cQ, L1 = self.cQ, level + 1
        pt = np.asarray(pt, dtype=np.uint64)[:L1]
        if fast:
            u = cQ.ntt(expand_ternary(self.oracle, self.Q[:L1], coeff_bits, sign_bits, self.N), level)   # :187
            c0 = cQ.ewise("MUL_MONT", u, np.asarray(pk0)[:L1])                                           # :190
            c1 = cQ.ewise("MUL_MONT", u, np.asarray(pk1)[:L1])                                           # :192
            c0 = cQ.ewise("ADD", c0, self.sample_ntt(e0, level))                                         # :195-196
            c1 = cQ.ewise("ADD", c1, self.sample_ntt(e1, level))                                         # :199-200
        else:
            ctx, moduli = self._through_p()
            n = len(moduli)
            u = ctx.ntt(expand_ternary(self.oracle, moduli, coeff_bits, sign_bits, self.N))              # :206
            pool0 = ctx.ewise("MUL_MONT", u, np.asarray(pk0)[:n])                                        # :209
            pool1 = ctx.ewise("MUL_MONT", u, np.asarray(pk1)[:n])                                        # :211
            pool0, pool1 = ctx.intt(pool0), ctx.intt(pool1)                                              # :214-215
            pool0 = ctx.ewise("ADD", pool0, expand_gaussian(moduli, e0, self.N))                         # :218 SampleAndAdd
            pool1 = ctx.ewise("ADD", pool1, expand_gaussian(moduli, e1, self.N))                         # :220
            c0 = self.baseconverter.moddown_pq(level, pool0)                                             # :223
            c1 = self.baseconverter.moddown_pq(level, pool1)                                             # :226
            c0, c1 = cQ.ntt(c0, level), cQ.ntt(c1, level)                                                # :229-230
        return np.stack([cQ.ewise("ADD", c0, pt), c1])                                                   # :234

    def encrypt_sk(self, fast, level, sk, crp, e, pt):
        """crp = the uniform poly in the NTT domain; it is not modified (the reference's ModDownNTTPQ transforms its P rows in place)"""
        cQ, L1 = self.cQ, level + 1
        pt = np.asarray(pt, dtype=np.uint64)[:L1]
        crp = np.asarray(crp, dtype=np.uint64)
        if fast:
            c0 = cQ.ewise("MUL_MONT", crp[:L1], np.asarray(sk)[:L1])                                     # :324
            c0 = cQ.ewise("NEG", c0)                                                                     # :325 (q - x: a zero product gives q)
            c0 = cQ.ewise("ADD", c0, self.sample_ntt(e, level))                                          # :327-328
            c1 = crp[:L1].copy()                                                                         # :330
        else:
            ctx, moduli = self._through_p()
            n = len(moduli)
            pool0 = ctx.ewise("MUL_MONT", crp[:n], np.asarray(sk)[:n])                                   # :337
            pool0 = ctx.ewise("NEG", pool0)                                                              # :338
            pool0 = ctx.intt(pool0)                                                                      # :341
            pool0 = ctx.ewise("ADD", pool0, expand_gaussian(moduli, e, self.N))                          # :344
            c0 = self.baseconverter.moddown_pq(level, pool0)                                             # :348
            c1 = self.baseconverter.moddown_ntt_pq(level, crp[:n])                                       # :352 (on a copy)
            c0 = cQ.ntt(c0, level)                                                                       # :355
        return np.stack([cQ.ewise("ADD", c0, pt), c1])                                                   # :359


def expand_pk_operands(oracle, enc, coeff_bits, sign_bits, e0, e1):
    """what lr_ckks_encrypt_pk takes for the same decisions: u = SampleTernaryMontgomeryNTT over Q||P, e0 / e1 = the residues SampleAndAdd adds"""
    moduli = enc.Q + enc.P
    u = enc.cQP.ntt(expand_ternary(oracle, moduli, coeff_bits, sign_bits, enc.N))
    return u, expand_gaussian(moduli, e0, enc.N), expand_gaussian(moduli, e1, enc.N)


def decrypt(oracle, enc, level, ct, sk):
    """decryptor.Decrypt (ckks/decryptor.go:53-78) through the oracle's plan"""
    cP = oracle.Context(enc.N, enc.P if enc.P else enc.Q[:1])
    return oracle.CkksPlan(enc.cQ, cP).decrypt(level, np.asarray(ct, dtype=np.uint64)[:, :level + 1], np.asarray(sk, dtype=np.uint64)[:level + 1])
