"""Test helper (not a test module): the per-ciphertext protocols of dckks and dbfv restated line by line over the CPU oracle's ring
primitives -- Context.ntt / intt / ewise and BasisExtender.moddown_* -- one ciphertext at a time, after the sampling:

    dckks/keyswitching.go:62-94          CKSProtocol.GenShare, genShareDelta       (:99-108 AggregateShares, KeySwitch)
    dbfv/keyswitching.go:74-109          the same for BFV                          (:114-122)
    dckks/public_keyswitching.go:63-93   PCKSProtocol.GenShare                     (:99-113)
    dbfv/public_keyswitching.go:111-148  the same for BFV                          (:154-165)

The samplers' decisions arrive in the compact form of the encryptors and are expanded by tests/bfv_encryptor_ref.py's rules; the smudging
sampler and the regular one differ only in the bytes the caller drew.  Keys are [|Q| + |P|, N] uint64 over contextQP, Q first, in NTT +
Montgomery form (the secret keys are read on the rows of Q); CKKS c1 and shares are in the NTT domain over limbs 0 .. level, BFV c1 and
shares in the coefficient domain over all of Q."""
import numpy as np

from bfv_encryptor_ref import expand_gaussian, expand_ternary

# Three parties, additive secret shares, a ciphertext under the collective public key, three shares with sigma = 6.36 bytes, the fold,
# KeySwitch, Decrypt, Decode at PN12QP109, scale 2^30 (tests/test_oracle_collective.py): the largest slot error over seeds 0 .. 2, both
# protocols, top level and level 0, measured on the CPU, and what the tests allow -- 16 x that, the margin of keygen_ref.CHAIN_TOLERANCE
# for its reason: the spread of the sampler draws across seeds.
SWITCH_MEASURED = 2.578290e-04
SWITCH_TOLERANCE = 16 * SWITCH_MEASURED
SWITCH_PARAMS, SWITCH_SCALE, SWITCH_SIGMA, SWITCH_PARTIES = "PN12QP109", 2.0 ** 30, 6.36, 3
BFV_T = 65537


class Collective:
    """what NewCKSProtocol / NewPCKSProtocol build (dckks/keyswitching.go:28-49, dbfv/public_keyswitching.go:76-97) for (N, Q, P)"""

    def __init__(self, oracle, N, Q, P):
        self.oracle, self.N = oracle, int(N)
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.moduli = self.Q + self.P
        self.cQ, self.cP = oracle.Context(N, self.Q), oracle.Context(N, self.P)
        self.cQP = oracle.Context(N, self.moduli)
        self.baseconverter = oracle.BasisExtender(self.cQ, self.cP)
        self.Pbig = 1
        for p in self.P:
            self.Pbig *= p

    def _mul_by_p(self, p, level):
        """Context.MulScalarBigintLvl(level, p, contextP.ModulusBigint) (ring/ring.go:541-552)"""
        return self.cQ.ewise("MUL_SCALAR_LIMBS", p, scalars=[self.Pbig % q for q in self.Q], level=level)

    # ---- CKS ----
    def ckks_cks_share(self, level, sk_in, sk_out, c1, e_bytes):
        cQ, nQ, L1 = self.cQ, len(self.Q), level + 1
        delta = cQ.ewise("SUB", np.asarray(sk_in)[:nQ], np.asarray(sk_out)[:nQ])                  # :64 Sub over all of Q
        share = cQ.ewise("MUL_MONT", np.asarray(c1)[:L1], delta[:L1])                             # :74 MulCoeffsMontgomeryLvl
        share = self._mul_by_p(share, level)                                                      # :76
        tmp = self.cQP.ntt(expand_gaussian(self.moduli, e_bytes, self.N))                         # :79 SampleNTT over Q||P
        share = cQ.ewise("ADD", share, tmp[:L1])                                                  # :80 AddLvl
        hP = tmp[nQ:].copy()                                                                      # :82-88 += onto zero
        return self.baseconverter.moddown_split_ntt_pq(level, share, hP)                          # :90

    def bfv_cks_share(self, sk_in, sk_out, c1, e_bytes, hp_zero=False):
        """hp_zero: the residue p_j that (magnitude 0, sign 0) leaves in hP written as 0 (what the device feeds the ModDown)"""
        cQ, nQ = self.cQ, len(self.Q)
        delta = cQ.ewise("SUB", np.asarray(sk_in)[:nQ], np.asarray(sk_out)[:nQ])                  # :76
        tmp = cQ.ntt(np.asarray(c1)[:nQ])                                                         # :88
        share = cQ.ewise("MUL_MONT", tmp, delta)                                                  # :89
        share = self._mul_by_p(share, nQ - 1)                                                     # :90
        share = cQ.intt(share)                                                                    # :92
        tmp = expand_gaussian(self.moduli, e_bytes, self.N)                                       # :94 Sample over Q||P
        share = cQ.ewise("ADD", share, tmp[:nQ])                                                  # :95
        hP = tmp[nQ:].copy()                                                                      # :97-103 += onto zero: p_j stays p_j
        if hp_zero:
            hP = np.where(hP == np.array(self.P, dtype=np.uint64)[:, None], np.uint64(0), hP)
        return self.baseconverter.moddown_split_pq(nQ - 1, share, hP)                             # :105

    # ---- PCKS ----
    def ckks_pcks_share(self, level, sk, pk0, pk1, c1, coeff_bits, sign_bits, e0, e1):
        ctx, cQ, n, L1 = self.cQP, self.cQ, len(self.moduli), level + 1
        tmp = ctx.ntt(expand_ternary(self.oracle, self.moduli, coeff_bits, sign_bits, self.N))    # :68
        share0 = ctx.ewise("MUL_MONT", tmp, np.asarray(pk0)[:n])                                  # :71
        share1 = ctx.ewise("MUL_MONT", tmp, np.asarray(pk1)[:n])                                  # :73
        share0 = ctx.ewise("ADD", share0, ctx.ntt(expand_gaussian(self.moduli, e0, self.N)))      # :76-77
        share1 = ctx.ewise("ADD", share1, ctx.ntt(expand_gaussian(self.moduli, e1, self.N)))      # :79-80
        out0 = self.baseconverter.moddown_ntt_pq(level, share0)                                   # :83
        out1 = self.baseconverter.moddown_ntt_pq(level, share1)                                   # :87
        out0 = cQ.ewise("MUL_MONT_AND_ADD", np.asarray(c1)[:L1], np.asarray(sk)[:L1], out=out0)   # :90
        return np.stack([out0, out1])

    def bfv_pcks_share(self, sk, pk0, pk1, c1, coeff_bits, sign_bits, e0, e1):
        ctx, cQ, n, nQ = self.cQP, self.cQ, len(self.moduli), len(self.Q)
        tmp = ctx.ntt(expand_ternary(self.oracle, self.moduli, coeff_bits, sign_bits, self.N))    # :116
        share0 = ctx.ewise("MUL_MONT", tmp, np.asarray(pk0)[:n])                                  # :119
        share1 = ctx.ewise("MUL_MONT", tmp, np.asarray(pk1)[:n])                                  # :121
        share0, share1 = ctx.intt(share0), ctx.intt(share1)                                       # :123-124
        share0 = ctx.ewise("ADD", share0, expand_gaussian(self.moduli, e0, self.N))               # :127 SampleAndAdd
        share1 = ctx.ewise("ADD", share1, expand_gaussian(self.moduli, e1, self.N))               # :129
        out0 = self.baseconverter.moddown_pq(nQ - 1, share0)                                      # :132
        out1 = self.baseconverter.moddown_pq(nQ - 1, share1)                                      # :136
        tmp = cQ.ntt(np.asarray(c1)[:nQ])                                                         # :139
        tmp = cQ.ewise("MUL_MONT", tmp, np.asarray(sk)[:nQ])                                      # :140
        tmp = cQ.intt(tmp)                                                                        # :141
        return np.stack([cQ.ewise("ADD", out0, tmp), out1])                                       # :144

    # ---- AggregateShares and KeySwitch of all four protocols ----
    def aggregate(self, shares, base=None):
        """AggregateShares folded over the parties in their order (dckks/keyswitching.go:99-101), then KeySwitch's Add onto ct[0]
        (:106); one share and no base is the Copy (:107, public_keyswitching.go:112)"""
        acc = np.array(shares[0], dtype=np.uint64)
        level = acc.shape[0] - 1
        for s in shares[1:]:
            acc = self.cQ.ewise("ADD", acc, np.asarray(s)[:level + 1])
        if base is not None:
            acc = self.cQ.ewise("ADD", np.asarray(base)[:level + 1], acc)
        return acc

    def cks_key_switch(self, combined, ct):
        """CKSProtocol.KeySwitch (dckks/keyswitching.go:104-108, dbfv/keyswitching.go:119-122)"""
        return np.stack([self.aggregate([combined], base=ct[0]), np.asarray(ct[1])[:combined.shape[0]]])

    def pcks_key_switch(self, combined, ct):
        """PCKSProtocol.KeySwitch (dckks/public_keyswitching.go:107-113, dbfv/public_keyswitching.go:161-165)"""
        return np.stack([self.aggregate([combined[0]], base=ct[0]), np.asarray(combined[1])])


def smudging_bytes(rng, shape, sigma=SWITCH_SIGMA):
    """decisions of a KYSampler with (sigma, bound = int(6 sigma)): a rounded normal, redrawn beyond the bound; magnitude | sign << 7,
    sign 1 = positive.  Not the reference's bit stream -- the protocol only needs the distribution."""
    bound = int(6 * sigma)
    v = np.rint(rng.normal(0.0, sigma, shape)).astype(np.int64)
    while True:
        bad = np.abs(v) > bound
        if not bad.any():
            break
        v[bad] = np.rint(rng.normal(0.0, sigma, int(bad.sum()))).astype(np.int64)
    sign = np.where(v == 0, rng.integers(0, 2, shape), v > 0).astype(np.int64)
    return (np.abs(v) | (sign << 7)).astype(np.uint8)


def edge_bytes(e):
    """the edge decisions at fixed positions: (0, +) (0, -) (19, +-) (127, +-)"""
    e = np.array(e, dtype=np.uint8)
    e[..., :6] = [0x80, 0, 19 | 0x80, 19, 127 | 0x80, 127]
    return e


def _planes(rng, N):
    return rng.integers(0, 256, N >> 3).astype(np.uint8), rng.integers(0, 256, N >> 3).astype(np.uint8)


def _regular_bytes(rng, shape):
    """decisions of the regular sampler (sigma 3.2, bound 19), as the encryptors' tests draw them"""
    return (rng.integers(0, 20, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)


def switch_inputs(N, Q, P, seed, parties=SWITCH_PARTIES):
    """everything one run of a protocol draws, in one place, so that the device test feeds the same bytes"""
    rng = np.random.default_rng(2000 + seed)
    QP, slots = list(Q) + list(P), N >> 1
    uniform = lambda: np.array([rng.integers(0, int(q), N, dtype=np.uint64) for q in QP], dtype=np.uint64)
    return {"sk_bits": [_planes(rng, N) for _ in range(parties)], "sk_out_bits": [_planes(rng, N) for _ in range(parties)],
            "pk_e": _regular_bytes(rng, N), "pk1": uniform(),
            "tgt_bits": _planes(rng, N), "tgt_e": _regular_bytes(rng, N), "tgt_pk1": uniform(),
            "enc_u": _planes(rng, N), "enc_e": (_regular_bytes(rng, N), _regular_bytes(rng, N)),
            "cks_e": smudging_bytes(rng, (parties, N)),
            "pcks_u": [_planes(rng, N) for _ in range(parties)],
            "pcks_e": [(smudging_bytes(rng, N), _regular_bytes(rng, N)) for _ in range(parties)],
            "values": rng.uniform(0, 1, slots) * np.exp(2j * np.pi * rng.uniform(0, 1, slots)),
            "ints": rng.integers(0, BFV_T, N).astype(np.uint64)}


def oracle_switch(oracle, scheme, protocol, N, Q, P, seed, level=None, roots=None):
    """parties with additive secret shares -> the collective public key of the summed secret (keygen_ref) -> a ciphertext under it ->
    one share per party -> the fold -> KeySwitch -> Decrypt under the summed output secret (cks) or the target secret (pcks) -> Decode, on
    the restatements.  Returns the inputs, the keys, the ciphertexts, the shares and the decoded values."""
    import bfv_encoder_ref
    import bfv_encryptor_ref
    import ckks_encoder_ref
    import ckks_encryptor_ref
    import keygen_ref
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    top = len(Q) - 1
    level = top if level is None or scheme == "bfv" else level
    d = switch_inputs(N, Q, P, seed)
    kg, col = keygen_ref.KeyGenerator(oracle, N, Q, P, scheme), Collective(oracle, N, Q, P)

    def total(keys):
        acc = keys[0]
        for k in keys[1:]:
            acc = kg.ctx.ewise("ADD", acc, k)
        return acc
    sks = [kg.gen_secret_key(*b) for b in d["sk_bits"]]
    sk = total(sks)
    pk0, pk1 = kg.gen_public_key(sk, d["pk_e"], d["pk1"]), d["pk1"]
    if scheme == "ckks":
        coder, enc = ckks_encoder_ref.Encoder(oracle, N, Q, roots), ckks_encryptor_ref.Encryptor(oracle, N, Q, P)
        pt = coder.encode(d["values"], top, SWITCH_SCALE)
        ct = enc.encrypt_pk(False, top, pk0, pk1, d["enc_u"][0], d["enc_u"][1], d["enc_e"][0], d["enc_e"][1], pt)[:, :level + 1]
    else:
        coder, enc = bfv_encoder_ref.Encoder(oracle, N, Q, BFV_T), bfv_encryptor_ref.Encryptor(oracle, N, Q, P)
        ct = enc.encrypt_pk(False, pk0, pk1, d["enc_u"][0], d["enc_u"][1], d["enc_e"][0], d["enc_e"][1], coder.encode_uint(d["ints"]))
    ct = np.ascontiguousarray(ct)
    if protocol == "cks":
        sk_outs = [kg.gen_secret_key(*b) for b in d["sk_out_bits"]]
        key = total(sk_outs)
        if scheme == "ckks":
            shares = [col.ckks_cks_share(level, sks[i], sk_outs[i], ct[1], d["cks_e"][i]) for i in range(len(sks))]
        else:
            shares = [col.bfv_cks_share(sks[i], sk_outs[i], ct[1], d["cks_e"][i]) for i in range(len(sks))]
        out = col.cks_key_switch(col.aggregate(shares), ct)
        d.update(sk_outs=sk_outs)
    else:
        key = kg.gen_secret_key(*d["tgt_bits"])
        tgt0, tgt1 = kg.gen_public_key(key, d["tgt_e"], d["tgt_pk1"]), d["tgt_pk1"]
        args = lambda i: (d["pcks_u"][i][0], d["pcks_u"][i][1], d["pcks_e"][i][0], d["pcks_e"][i][1])
        if scheme == "ckks":
            shares = [col.ckks_pcks_share(level, sks[i], tgt0, tgt1, ct[1], *args(i)) for i in range(len(sks))]
        else:
            shares = [col.bfv_pcks_share(sks[i], tgt0, tgt1, ct[1], *args(i)) for i in range(len(sks))]
        combined = np.stack([col.aggregate([s[0] for s in shares]), col.aggregate([s[1] for s in shares])])
        out = col.pcks_key_switch(combined, ct)
        d.update(tgt0=tgt0, tgt1=tgt1)
    if scheme == "ckks":
        decoded = coder.decode(ckks_encryptor_ref.decrypt(oracle, enc, level, out, key), N >> 1, level, SWITCH_SCALE)
    else:
        decoded = coder.decode_uint(bfv_encryptor_ref.decrypt(enc.cQ, out, key))
    d.update(sks=sks, sk=sk, pk0=pk0, pk1=pk1, ct=ct, shares=shares, out=out, key=key, decoded=decoded, level=level)
    return d
