"""Test helper (not a test module): the collective Refresh of dckks and dbfv restated line by line over the CPU oracle's ring primitives --
Context.ntt / intt / ewise, BasisExtender.moddown_* and SimpleScaler.scale -- one ciphertext at a time, after the sampling:

    dckks/public_refresh.go   GenShares :43-95 (from :66 on)   Aggregate :98   Decrypt :103   Recode :108-139   Recrypt :142-147
    dbfv/public_refresh.go    GenShares :105-160   Aggregate :163   Decrypt :169   Recode :174-179   Recrypt :182-190   Finalize :193-197
                              lift :199-205

The big-integer lines (SetCoefficientsBigint(Lvl), PolyToBigint, the centring) are Python integers.  The noise arrives in the compact form
of the encryptors and is expanded by tests/bfv_encryptor_ref.py's rule.  The CKKS mask is a list of N Python integers (what ring.RandInt
gives, centred, :58-62), the BFV mask a row of N values below t.  sk is [|Q| (+ |P|), N] uint64 in NTT + Montgomery form; CKKS polys are
in the NTT domain, BFV polys in the coefficient domain (crs over Q||P).  The *_default methods restate the device's default shapes in
their order; tests/test_oracle_refresh.py pins that they give the same bits."""
import numpy as np

from bfv_encryptor_ref import expand_gaussian

# Three parties with additive secret shares at PN12QP109, scale 2^30: a ciphertext under the collective public key at levelStart 0 and 1,
# three pairs of shares (sigma 3.19 bytes, masks uniform below Q_levelStart / 6, centred), Aggregate, Decrypt, Recode, Recrypt, decryption
# at level L, Decode (tests/test_oracle_refresh.py): the largest slot error over seeds 0 .. 2 and both levels, measured on the CPU
# restatement, and what the tests allow -- 16 x that, the margin of collective_ref.SWITCH_TOLERANCE for its reason: the spread of the
# sampler draws across seeds.
REFRESH_MEASURED = 9.327266e-05
REFRESH_TOLERANCE = 16 * REFRESH_MEASURED
REFRESH_PARAMS, REFRESH_SCALE, REFRESH_PARTIES = "PN12QP109", 2.0 ** 30, 3
BFV_T = 65537


def product(values):
    out = 1
    for v in values:
        out *= int(v)
    return out


def centre(v, bound):
    """:59-62 and :130-133: Cmp(bound >> 1) is 1 or 0 => v -= bound"""
    return v - bound if v >= bound >> 1 else v


def mask_words(Q, level_start):
    """the 64-bit words that hold Q_levelStart: every centred mask below it fits them in two's complement"""
    return -(-product(Q[:level_start + 1]).bit_length() // 64)


def reduce_words(words, q):
    """the device's SetCoefficientsBigint on one coefficient: `words` little-endian 64-bit words of a two's complement integer -> its
    Euclidean residue, word by word from the top, every step on values below 2^64 (the top word is signed: top - 2^64)"""
    two64 = (1 << 64) % q
    r = int(words[-1]) % q
    if int(words[-1]) >> 63:
        r = (r + q - two64) % q
    for w in reversed([int(x) for x in words[:-1]]):
        r = (r * two64 % q + w % q) % q
    return r


def garner_recode(Q, level_start, residues):
    """the device's Recode on one coefficient (csrc/lr_refresh.hip): mixed-radix digits of the CRT of residues[0 .. levelStart], the
    comparison with the digits of Q_ls >> 1 from the top, and v mod q_i as a Horner chain; every value below 2^64"""
    ls = level_start
    d = []
    for k in range(ls + 1):
        q, u = Q[k], 0
        for m in range(k - 1, -1, -1):
            u = (u * (Q[m] % q) + d[m] % q) % q
        inv = pow(product(Q[:k]) % q, -1, q) if k else 1
        d.append((int(residues[k]) % q - u) % q * inv % q if k else int(residues[0]) % q)
    H, h = product(Q[:ls + 1]) >> 1, []
    for k in range(ls + 1):
        h.append(H % Q[k])
        H //= Q[k]
    neg = True
    for k in range(ls, -1, -1):
        if d[k] != h[k]:
            neg = d[k] > h[k]
            break
    out = []
    for q in Q:
        r = 0
        for k in range(ls, -1, -1):
            r = (r * (Q[k] % q) + d[k] % q) % q
        out.append((r + q - product(Q[:ls + 1]) % q) % q if neg else r)
    return out


class Refresh:
    """what the two NewRefreshProtocol constructors build (dckks/public_refresh.go:23-35, dbfv/public_refresh.go:79-96) for (N, Q, P, t);
    P empty or t = 0: the CKKS protocol only"""

    def __init__(self, oracle, N, Q, P=(), t=0):
        self.oracle, self.N, self.t = oracle, int(N), int(t)
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.moduli = self.Q + self.P
        self.cQ = oracle.Context(N, self.Q)
        if self.P:
            self.cP, self.cQP = oracle.Context(N, self.P), oracle.Context(N, self.moduli)
            self.baseconverter = oracle.BasisExtender(self.cQ, self.cP)
            self.Pbig = product(self.P)
        if self.t:
            self.scaler = oracle.SimpleScaler(self.t, self.cQ)
            delta = product(self.Q) // self.t
            self.delta_mont = [oracle.mform(delta % q, q) for q in self.Q]                        # dbfv/dbfv.go: deltaMont

    # ---- the big-integer lines ----
    def set_coefficients_bigint(self, coeffs, limbs):
        """SetCoefficientsBigintLvl(limbs - 1, coeffs, p) (ring/ring_context.go:356-367): big.Int.Mod is Euclidean, as Python's %"""
        return np.array([[int(c) % q for c in coeffs] for q in self.Q[:limbs]], dtype=np.uint64)

    def poly_to_bigint(self, p):
        """PolyToBigint (ring/ring_context.go:384-421) of a poly of level = rows - 1: crtReconstruction is built from the whole modulus,
        the sum is reduced modulo Q_level"""
        p = np.asarray(p, dtype=np.uint64)
        rows, Qfull, Qlevel = p.shape[0], product(self.Q), product(self.Q[:p.shape[0]])
        crt = []
        for i in range(rows):
            qhat = Qfull // self.Q[i]
            crt.append(qhat * pow(qhat % self.Q[i], -1, self.Q[i]))
        return [sum(int(p[i, x]) * crt[i] for i in range(rows)) % Qlevel for x in range(self.N)]

    # ---- dckks ----
    def ckks_gen_shares(self, level_start, sk, c1, crs, mask, e0, e1):
        cQ, nQ, L1 = self.cQ, len(self.Q), level_start + 1
        sk = np.asarray(sk, dtype=np.uint64)[:nQ]
        dec = self.set_coefficients_bigint(mask, L1)                                              # :66
        rec = self.set_coefficients_bigint(mask, nQ)                                              # :68
        dec, rec = cQ.ntt(dec), cQ.ntt(rec)                                                       # :74-75
        dec = cQ.ewise("MUL_MONT_AND_ADD", sk[:L1], np.asarray(c1)[:L1], out=dec)                 # :78
        rec = cQ.ewise("MUL_MONT_AND_ADD", sk, np.asarray(crs)[:nQ], out=rec)                     # :81
        tmp = cQ.ntt(expand_gaussian(self.Q, e0, self.N))                                         # :84 SampleNTT
        dec = cQ.ewise("ADD", dec, tmp[:L1])                                                      # :85
        tmp = cQ.ntt(expand_gaussian(self.Q, e1, self.N))                                         # :88
        rec = cQ.ewise("ADD", rec, tmp)                                                           # :89
        return dec, cQ.ewise("NEG", rec)                                                          # :92

    def ckks_gen_shares_default(self, level_start, sk, c1, crs, mask, e0, e1):
        """the device's default shape: the mask reduced and transformed once over all of Q, e0 on limbs 0 .. levelStart only, the (0, sign
        0) residue written as 0 in front of the transforms"""
        cQ, nQ, L1 = self.cQ, len(self.Q), level_start + 1
        sk = np.asarray(sk, dtype=np.uint64)[:nQ]
        zeroed = lambda p, moduli: np.where(p == np.array(moduli, dtype=np.uint64)[:, None], np.uint64(0), p)
        m = cQ.ntt(self.set_coefficients_bigint(mask, nQ))
        n0 = cQ.ntt(zeroed(expand_gaussian(self.Q[:L1], e0, self.N), self.Q[:L1]))
        n1 = cQ.ntt(zeroed(expand_gaussian(self.Q, e1, self.N), self.Q))
        dec = cQ.ewise("ADD", cQ.ewise("MUL_MONT_AND_ADD", sk[:L1], np.asarray(c1)[:L1], out=m[:L1]), n0)
        rec = cQ.ewise("ADD", cQ.ewise("MUL_MONT_AND_ADD", sk, np.asarray(crs)[:nQ], out=m), n1)
        return dec, cQ.ewise("NEG", rec)

    def ckks_recode_integers(self, p_in):
        """:112-134: the centred integers of a poly in the NTT domain"""
        p_in = np.asarray(p_in, dtype=np.uint64)
        Qstart = product(self.Q[:p_in.shape[0]])                                                  # :116-119
        return [centre(v, Qstart) for v in self.poly_to_bigint(self.cQ.intt(p_in))]               # :112, :114, :121-134

    def ckks_recode(self, p_in):
        """Recode of a poly with levelStart + 1 rows: all of Q"""
        return self.cQ.ntt(self.set_coefficients_bigint(self.ckks_recode_integers(p_in), len(self.Q)))   # :136, :138

    def ckks_recode_default(self, p_in):
        """the device's default shape: rows 0 .. levelStart copied, the new rows alone computed and transformed"""
        p_in = np.asarray(p_in, dtype=np.uint64)
        L1, nQ = p_in.shape[0], len(self.Q)
        out = np.zeros((nQ, self.N), dtype=np.uint64)
        out[:L1] = p_in
        if L1 < nQ:
            coeffs = self.ckks_recode_integers(p_in)
            new = np.array([[c % q for c in coeffs] for q in self.Q[L1:]], dtype=np.uint64)
            out[L1:] = self.oracle.Context(self.N, self.Q[L1:]).ntt(new)
        return out

    def ckks_finalize(self, level_start, c0, dec, rec, recode=None):
        L1 = level_start + 1
        p = self.cQ.ewise("ADD", np.asarray(c0)[:L1], np.asarray(dec)[:L1])                       # :104
        p = (recode or self.ckks_recode)(p)                                                       # :108-139
        return self.cQ.ewise("ADD", p, np.asarray(rec))                                           # :144; ct[1] = crs.CopyNew() (:146)

    # ---- dbfv ----
    def lift(self, row):
        """:199-205: p1.Coeffs[i][j] = MRed(p0.Coeffs[0][j], deltaMont[i], q_i); a value >= t goes through as it is"""
        row = np.ascontiguousarray(row, dtype=np.uint64).reshape(self.N)
        lifted = np.broadcast_to(row, (len(self.Q), self.N)).copy()
        delta = np.broadcast_to(np.array(self.delta_mont, dtype=np.uint64)[:, None], (len(self.Q), self.N)).copy()
        return self.cQ.ewise("MUL_MONT", lifted, delta)

    def bfv_gen_shares(self, sk, c1, crs, mask, e0, e1, hp_zero=False):
        """as the first call on a fresh RefreshProtocol: rfp.hP starts at zero (the reference never zeroes it again).  hp_zero: the residue
        p_j that (magnitude 0, sign 0) leaves in hP written as 0 (what the device's default shape feeds the ModDown)"""
        cQ, ctx, nQ, n = self.cQ, self.cQP, len(self.Q), len(self.moduli)
        sk, level = np.asarray(sk, dtype=np.uint64)[:n], nQ - 1
        tmp1 = cQ.ntt(np.asarray(c1)[:nQ])                                                        # :116
        dec = cQ.ewise("MUL_MONT", sk[:nQ], tmp1)                                                 # :117
        dec = cQ.intt(dec)                                                                        # :119
        dec = cQ.ewise("MUL_SCALAR_LIMBS", dec, scalars=[self.Pbig % q for q in self.Q], level=level)   # :122
        tmp1 = expand_gaussian(self.moduli, e0, self.N)                                           # :125 Sample over Q||P
        dec = cQ.ewise("ADD", dec, tmp1[:nQ])                                                     # :126
        hP = tmp1[nQ:].copy()                                                                     # :128-134 += onto zero: p_j stays p_j
        if hp_zero:
            hP = np.where(hP == np.array(self.P, dtype=np.uint64)[:, None], np.uint64(0), hP)
        dec = self.baseconverter.moddown_split_pq(level, dec, hP)                                 # :137
        tmp1 = ctx.ntt(np.asarray(crs)[:n])                                                       # :140
        tmp2 = ctx.ewise("MUL_MONT", sk, tmp1)                                                    # :141
        tmp2 = ctx.ewise("NEG", tmp2)                                                             # :142
        tmp2 = ctx.intt(tmp2)                                                                     # :143
        tmp2 = ctx.ewise("ADD", tmp2, expand_gaussian(self.moduli, e1, self.N))                   # :146 SampleAndAdd
        rec = self.baseconverter.moddown_pq(level, tmp2)                                          # :149
        tmp1 = self.lift(mask)                                                                    # :152-153
        return cQ.ewise("ADD", dec, tmp1), cQ.ewise("SUB", rec, tmp1)                             # :156, :159

    def bfv_finalize(self, c0, crs, dec, rec):
        cQ, nQ = self.cQ, len(self.Q)
        tmp1 = cQ.ewise("ADD", np.asarray(c0)[:nQ], np.asarray(dec)[:nQ])                         # :170
        tmp1 = self.scaler.scale(tmp1, nQ)                                                        # :177
        tmp1 = self.lift(tmp1[0])                                                                 # :178
        out0 = cQ.ewise("ADD", tmp1, np.asarray(rec)[:nQ])                                        # :185
        return np.stack([out0, self.baseconverter.moddown_pq(nQ - 1, np.asarray(crs)[:len(self.moduli)])])   # :188

    # ---- Aggregate of both protocols over the parties in their order ----
    def aggregate(self, shares):
        acc = np.array(shares[0], dtype=np.uint64)
        for s in shares[1:]:
            acc = self.cQ.ewise("ADD", acc, np.asarray(s)[:acc.shape[0]])                         # dckks :99, dbfv :164-165
        return acc


def regular_bytes(rng, shape):
    """decisions of the references' sampler (sigma 3.19, bound int(6 sigma) = 19), drawn as collective_ref.smudging_bytes draws its own"""
    import collective_ref
    return collective_ref.smudging_bytes(rng, shape, sigma=3.19)


def draw_mask(rng, bound, N):
    """ring.RandInt(bound) per coefficient, centred (:57-63)"""
    nbytes = (bound.bit_length() + 7) // 8 + 8
    return [centre(int.from_bytes(rng.bytes(nbytes), "little") % bound, bound) for _ in range(N)]


def _planes(rng, N):
    return rng.integers(0, 256, N >> 3).astype(np.uint8), rng.integers(0, 256, N >> 3).astype(np.uint8)


def refresh_inputs(scheme, N, Q, P, seed, level_start, parties=REFRESH_PARTIES):
    """everything one run draws, in one place, so that the device test feeds the same bytes"""
    rng = np.random.default_rng(3000 + seed)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    QP, slots = Q + P, N >> 1
    uniform = lambda moduli: np.array([rng.integers(0, q, N, dtype=np.uint64) for q in moduli], dtype=np.uint64)
    d = {"sk_bits": [_planes(rng, N) for _ in range(parties)], "pk_e": regular_bytes(rng, N), "pk1": uniform(QP),
         "enc_u": _planes(rng, N), "enc_e": (regular_bytes(rng, N), regular_bytes(rng, N)),
         "e": [(regular_bytes(rng, N), regular_bytes(rng, N)) for _ in range(parties)]}
    if scheme == "ckks":
        bound = product(Q[:level_start + 1]) // (2 * parties)                                     # :48-53
        d["crs"] = uniform(Q)
        d["mask"] = [draw_mask(rng, bound, N) for _ in range(parties)]
        d["values"] = rng.uniform(0, 1, slots) * np.exp(2j * np.pi * rng.uniform(0, 1, slots))
    else:
        d["crs"] = uniform(QP)
        d["mask"] = [rng.integers(0, BFV_T, N).astype(np.uint64) for _ in range(parties)]
        d["ints"] = rng.integers(0, BFV_T, N).astype(np.uint64)
        d["factor"] = rng.integers(0, BFV_T, N).astype(np.uint64)                                 # the plaintext operand of the product, by slots
    return d


def bfv_noise(ref, ct, sk, expected):
    """the largest centred coefficient of c0 + c1 s - floor(Q / t) m over Python integers: the noise of a degree-1 ciphertext"""
    import bfv_encryptor_ref
    cQ, Qbig = ref.cQ, product(ref.Q)
    phase = bfv_encryptor_ref.decrypt(cQ, ct, sk)
    coeffs = ref.poly_to_bigint(phase)
    delta = Qbig // ref.t
    return max(abs(centre((c - delta * int(m)) % Qbig, Qbig)) for c, m in zip(coeffs, expected))


def oracle_refresh(oracle, scheme, N, Q, P, seed, level_start=None, roots=None):
    """parties with additive secret shares -> the collective public key -> a ciphertext under it (CKKS: dropped to levelStart; BFV:
    multiplied by a plaintext poly, the product that is refreshed) -> one pair of shares per party -> Aggregate -> Decrypt, Recode, Recrypt
    -> decryption under the summed secret -> Decode, on the restatements.  Returns the inputs, keys, ciphertexts, shares and decoded values."""
    import bfv_encoder_ref
    import bfv_encryptor_ref
    import ckks_encoder_ref
    import ckks_encryptor_ref
    import keygen_ref
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    top = len(Q) - 1
    level_start = top if level_start is None or scheme == "bfv" else level_start
    d = refresh_inputs(scheme, N, Q, P, seed, level_start)
    kg = keygen_ref.KeyGenerator(oracle, N, Q, P, scheme)
    ref = Refresh(oracle, N, Q, P, BFV_T if scheme == "bfv" else 0)
    sks = [kg.gen_secret_key(*b) for b in d["sk_bits"]]
    sk = sks[0]
    for k in sks[1:]:
        sk = kg.ctx.ewise("ADD", sk, k)
    pk0, pk1 = kg.gen_public_key(sk, d["pk_e"], d["pk1"]), d["pk1"]
    n = len(sks)
    if scheme == "ckks":
        coder, enc = ckks_encoder_ref.Encoder(oracle, N, Q, roots), ckks_encryptor_ref.Encryptor(oracle, N, Q, P)
        pt = coder.encode(d["values"], top, REFRESH_SCALE)
        ct = enc.encrypt_pk(False, top, pk0, pk1, d["enc_u"][0], d["enc_u"][1], d["enc_e"][0], d["enc_e"][1], pt)[:, :level_start + 1]
        ct = np.ascontiguousarray(ct)
        shares = [ref.ckks_gen_shares(level_start, sks[i], ct[1], d["crs"], d["mask"][i], *d["e"][i]) for i in range(n)]
        dec, rec = ref.aggregate([s[0] for s in shares]), ref.aggregate([s[1] for s in shares])
        out = np.stack([ref.ckks_finalize(level_start, ct[0], dec, rec), d["crs"]])
        decoded = coder.decode(ckks_encryptor_ref.decrypt(oracle, enc, top, out, sk), N >> 1, top, REFRESH_SCALE)
    else:
        coder, enc = bfv_encoder_ref.Encoder(oracle, N, Q, BFV_T), bfv_encryptor_ref.Encryptor(oracle, N, Q, P)
        fresh = enc.encrypt_pk(False, pk0, pk1, d["enc_u"][0], d["enc_u"][1], d["enc_e"][0], d["enc_e"][1], coder.encode_uint(d["ints"]))
        # the product that is refreshed: both components times the plaintext poly of `factor` (coefficients below t, not scaled by
        # floor(Q / t)): the slots multiply
        cQ = enc.cQ
        row = coder.cT.intt(coder._scatter(d["factor"])[None])[0]
        f = cQ.ewise("MFORM", cQ.ntt(np.broadcast_to(row, (len(Q), N)).copy()))
        ct = np.stack([cQ.intt(cQ.ewise("MUL_MONT", cQ.ntt(c), f)) for c in fresh])
        d["fresh"] = fresh
        d["expected"] = d["ints"] * d["factor"] % np.uint64(BFV_T)
        d["expected_poly"] = coder.cT.intt(coder._scatter(d["expected"])[None])[0]
        shares = [ref.bfv_gen_shares(sks[i], ct[1], d["crs"], d["mask"][i], *d["e"][i]) for i in range(n)]
        dec, rec = ref.aggregate([s[0] for s in shares]), ref.aggregate([s[1] for s in shares])
        out = ref.bfv_finalize(ct[0], d["crs"], dec, rec)
        decoded = coder._decode(bfv_encryptor_ref.decrypt(cQ, out, sk))
    d.update(sks=sks, sk=sk, pk0=pk0, pk1=pk1, ct=ct, shares=shares, dec=dec, rec=rec, out=out, decoded=decoded, level_start=level_start,
             ref=ref)
    return d
