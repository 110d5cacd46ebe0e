"""Test helper (not a test module): the collective key setup of dbfv and dckks restated line by line over the CPU oracle's ring primitives
-- Context.ntt / ewise (ADD, SUB, COPY, MUL_MONT, MUL_MONT_AND_ADD, MUL_MONT_AND_SUB, MUL_SCALAR_LIMBS, INV_MFORM, MFORM) / permute_ntt --
one party at a time, after the sampling:

    dbfv/publickey_gen.go:54-67          CKGProtocol.GenShare, AggregateShares, GenPublicKey          (dckks/publickey_gen.go:39-55)
    dbfv/relinkey_gen.go:215-355         RKGProtocol, three rounds and GenRelinearizationKey          (dckks/relinkey_gen.go:65-223)
    dbfv/relinkey_gen_naive.go:59-200    RKGProtocolNaive, two rounds and GenRelinearizationKey       (dckks/relinkey_gen_naive.go:59-199)
    dbfv/rotkey_gen.go:139-215           RTGProtocol.genShare, Aggregate, Finalize                    (dckks/rotkey_gen.go:95-176)

scheme = "bfv" or "ckks" selects whose lines run; they differ in how the digit loop's break is spelt and in
dckks/relinkey_gen_naive.go:73-75, which draws both round-one noise polys into shareOut[i][0].  The samplers' decisions arrive in the
compact form of the encryptors and are expanded by tests/bfv_encryptor_ref.py's rules; crs and crp are arguments.  Polys are
[|Q| + |P|, N] uint64 over contextQP, Q first, in the NTT domain; sk, u and pk in Montgomery form.  A share of beta polys is
[beta, |Q| + |P|, N]; a share of beta pairs is [2 beta, |Q| + |P|, N], member 2 i = [i][0], member 2 i + 1 = [i][1] -- the layout the
oracle's key switch reads."""
import numpy as np

from bfv_encryptor_ref import expand_gaussian, expand_ternary
from keygen_ref import draw, uniform  # noqa: F401  (the tests draw through this module)

PARTIES = 3


class Setup:
    """what NewCKGProtocol, NewEkgProtocol, NewEkgProtocolNaive and NewRotKGProtocol build for (N, Q, P)"""

    def __init__(self, oracle, N, Q, P, scheme="bfv"):
        assert scheme in ("ckks", "bfv")
        self.oracle, self.N, self.scheme = oracle, int(N), scheme
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.moduli = self.Q + self.P
        self.ctx = oracle.Context(N, self.moduli)                                     # contextQP
        self.alpha = len(self.P)                                                      # params.Alpha()
        self.beta = -(-len(self.Q) // len(self.P)) if self.P else 0                   # params.Beta()
        self.Pbig = 1
        for p in self.P:
            self.Pbig *= p

    # ---- what the protocols share ----
    def sample_ntt(self, e_bytes):
        """gaussianSampler.SampleNTT: Sample over contextQP, then Context.NTT"""
        return self.ctx.ntt(expand_gaussian(self.moduli, e_bytes, self.N))

    def ternary_ntt(self, coeff_bits, sign_bits):
        """SampleTernaryMontgomeryNTT(0.5) over contextQP; NewEphemeralKey (dbfv/relinkey_gen.go:208) and GenSecretKey are this too"""
        return self.ctx.ntt(expand_ternary(self.oracle, self.moduli, coeff_bits, sign_bits, self.N))

    def times_p(self, p):
        """MulScalarBigint(p, contextP.ModulusBigint), InvMForm (dbfv/relinkey_gen.go:225-227)"""
        pool = self.ctx.ewise("MUL_SCALAR_LIMBS", p, scalars=[self.Pbig % q for q in self.moduli])
        return self.ctx.ewise("INV_MFORM", pool)

    def add_digit(self, x, pool, i, exact_break=False):
        """the loop over the rows of digit i with its break: dbfv/relinkey_gen.go:235-250 breaks at index == |Q| - 1, every other file at
        index >= |Q| - 1"""
        last = len(self.Q) - 1
        for j in range(self.alpha):
            index = i * self.alpha + j
            row = self.ctx.ewise("ADD", np.ascontiguousarray(x[:index + 1]), np.ascontiguousarray(pool[:index + 1]), level=index)
            x[index] = row[index]
            if (index == last) if exact_break else (index >= last):
                break
        return x

    def aggregate(self, shares):
        """every Aggregate*: Context.Add over contextQP, share after share"""
        acc = np.array(shares[0], dtype=np.uint64)
        for s in shares[1:]:
            acc = np.stack([self.ctx.ewise("ADD", a, b) for a, b in zip(acc, s)]) if acc.ndim == 3 else self.ctx.ewise("ADD", acc, s)
        return acc

    # ---- CKG ----
    def ckg_share(self, sk, crs, e_bytes):
        share = self.sample_ntt(e_bytes)                                              # publickey_gen.go:55
        return self.ctx.ewise("MUL_MONT_AND_SUB", sk, crs, out=share)                 # :56

    # ---- RKG, three rounds ----
    def rkg_round1(self, u, sk, crp, e_bytes):
        """e_bytes [beta, N]"""
        ctx = self.ctx
        pool = self.times_p(np.array(sk, dtype=np.uint64))                            # relinkey_gen.go:223-227
        out = []
        for i in range(self.beta):
            share = self.sample_ntt(e_bytes[i])                                       # :232
            share = self.add_digit(share, pool, i, exact_break=self.scheme == "bfv")  # :235-250 (dckks :88-103)
            out.append(ctx.ewise("MUL_MONT_AND_SUB", u, crp[i], out=share))           # :253
        return np.stack(out)

    def rkg_round2(self, round1, sk, crp, e_bytes):
        """e_bytes [beta, 2, N]"""
        ctx, out = self.ctx, []
        for i in range(self.beta):
            s0 = ctx.ewise("MUL_MONT", round1[i], sk)                                 # :286
            s0 = ctx.ewise("ADD", s0, self.sample_ntt(e_bytes[i][0]))                 # :289-290
            s1 = self.sample_ntt(e_bytes[i][1])                                       # :294
            s1 = ctx.ewise("MUL_MONT_AND_ADD", sk, crp[i], out=s1)                    # :296
            out += [s0, s1]
        return np.stack(out)

    def rkg_round3(self, round2, u, sk, e_bytes):
        """e_bytes [beta, N]"""
        ctx, out = self.ctx, []
        tmp = ctx.ewise("SUB", u, sk)                                                 # :325
        for i in range(self.beta):
            share = self.sample_ntt(e_bytes[i])                                       # :330
            out.append(ctx.ewise("MUL_MONT_AND_ADD", tmp, round2[2 * i + 1], out=share))      # :331
        return np.stack(out)

    def rkg_key(self, round2, round3):
        ctx, out = self.ctx, []
        for i in range(self.beta):
            k0 = ctx.ewise("ADD", round2[2 * i], round3[i])                           # :348
            k1 = np.array(round2[2 * i + 1], dtype=np.uint64)                         # :349
            out += [ctx.ewise("MFORM", k0), ctx.ewise("MFORM", k1)]                   # :351-352
        return np.stack(out)

    # ---- RKG, naive ----
    def naive_round1(self, sk, pk0, pk1, e_bytes, u_coeff_bits, u_sign_bits, share=None):
        """e_bytes [beta, 2, N], the planes [beta, N / 8]; share: what shareOut holds on entry (AllocateShares: zero)"""
        ctx, rows = self.ctx, len(self.moduli)
        share = np.zeros((2 * self.beta, rows, self.N), dtype=np.uint64) if share is None else np.array(share, dtype=np.uint64)
        pool = self.times_p(np.array(sk, dtype=np.uint64))                            # relinkey_gen_naive.go:63-67
        for i in range(self.beta):
            if self.scheme == "bfv":
                share[2 * i] = self.sample_ntt(e_bytes[i][0])                         # dbfv :74
                share[2 * i + 1] = self.sample_ntt(e_bytes[i][1])                     # dbfv :76
            else:
                share[2 * i] = self.sample_ntt(e_bytes[i][0])                         # dckks :73
                share[2 * i] = self.sample_ntt(e_bytes[i][1])                         # dckks :75: into [i][0] again
            share[2 * i] = self.add_digit(share[2 * i], pool, i)                      # :80-97
        for i in range(self.beta):
            t = self.ternary_ntt(u_coeff_bits[i], u_sign_bits[i])                     # :102
            share[2 * i] = ctx.ewise("MUL_MONT_AND_ADD", pk0, t, out=share[2 * i].copy())             # :104
            share[2 * i + 1] = ctx.ewise("MUL_MONT_AND_ADD", pk1, t, out=share[2 * i + 1].copy())     # :106
        return share

    def naive_round2(self, round1, sk, pk0, pk1, v_coeff_bits, v_sign_bits, e_bytes):
        ctx, out = self.ctx, []
        for i in range(self.beta):
            s0 = ctx.ewise("MUL_MONT", round1[2 * i], sk)                             # :143
            s1 = ctx.ewise("MUL_MONT", round1[2 * i + 1], sk)                         # :144
            t = self.ternary_ntt(v_coeff_bits[i], v_sign_bits[i])                     # :147
            s0 = ctx.ewise("MUL_MONT_AND_ADD", pk0, t, out=s0)                        # :150
            s1 = ctx.ewise("MUL_MONT_AND_ADD", pk1, t, out=s1)                        # :153
            s0 = ctx.ewise("ADD", s0, self.sample_ntt(e_bytes[i][0]))                 # :156-157
            s1 = ctx.ewise("ADD", s1, self.sample_ntt(e_bytes[i][1]))                 # :160-161
            out += [s0, s1]
        return np.stack(out)

    def naive_key(self, round2):
        return np.stack([self.ctx.ewise("MFORM", np.array(m, dtype=np.uint64)) for m in round2])       # :194-198

    # ---- RTG ----
    def rtg_share(self, sk, gen, crp, e_bytes):
        """genShare (rotkey_gen.go:139-184) for the Galois element gen; e_bytes [beta, N]"""
        ctx, out = self.ctx, []
        pool = self.times_p(ctx.permute_ntt(sk, gen))                                 # :143-146
        for i in range(self.beta):
            share = self.sample_ntt(e_bytes[i])                                       # :153
            share = self.add_digit(share, pool, i)                                    # :159-175
            share = ctx.ewise("MUL_MONT_AND_SUB", crp[i], sk, out=share)              # :178
            out.append(ctx.ewise("MFORM", share))                                     # :179
        return np.stack(out)

    def rtg_key(self, share, crp):
        out = []
        for i in range(self.beta):
            out += [np.array(share[i], dtype=np.uint64), self.ctx.ewise("MFORM", crp[i])]      # :210-211
        return np.stack(out)


def edge_noise(e):
    """the edge bytes at fixed positions of a [..., N] noise array (first poly): (0, sign 0), (0, sign 1), (19, +-), (127, +-), and
    (0, sign 0) on the last coefficient"""
    flat = e.reshape(-1, e.shape[-1])
    flat[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
    flat[-1, -1] = 0
    return e


def edge_planes(c, s):
    """the four ternary (coeff, sign) pairs in byte 0 of the first poly, and a plane of all ones in the last"""
    fc, fs = c.reshape(-1, c.shape[-1]), s.reshape(-1, s.shape[-1])
    fc[0, 0], fs[0, 0] = 0b10101010, 0b11001100
    fc[-1, :] = 0xFF
    return c, s


def edge_uniform(a, moduli):
    """coefficients 0 and q_j - 1 in the first poly of a uniform [..., rows, N] array"""
    flat = a.reshape(-1, a.shape[-2], a.shape[-1])
    flat[0, :, 2] = 0
    flat[0, :, -1] = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    return a


def inputs(N, Q, P, seed, parties=PARTIES, n_gens=1):
    """everything one full setup of `parties` parties draws, with the edge bytes at fixed positions"""
    rng = np.random.default_rng(7000 + seed)
    QP, beta, n = list(Q) + list(P), -(-len(Q) // len(P)), parties
    planes = lambda *shape: edge_planes(draw(rng, shape + (N >> 3,)), draw(rng, shape + (N >> 3,)))
    noise = lambda *shape: edge_noise(draw(rng, shape_noise=shape + (N,)))
    return {"sk_bits": planes(n), "u_bits": planes(n),
            "crs": edge_uniform(uniform(rng, QP, N), QP), "crp": edge_uniform(uniform(rng, QP, N, beta), QP),
            "crp_rot": edge_uniform(uniform(rng, QP, N, n_gens * beta).reshape(n_gens, beta, len(QP), N), QP),
            "ckg_e": noise(n), "r1_e": noise(n, beta), "r2_e": noise(n, beta, 2), "r3_e": noise(n, beta),
            "n1_e": noise(n, beta, 2), "n1_bits": planes(n, beta), "n2_e": noise(n, beta, 2), "n2_bits": planes(n, beta),
            "rtg_e": noise(n_gens, n, beta)}


def run_all(st, d, gens):
    """one full setup on the restatement: every party's share of every round, the aggregates and the keys.  Returns a dict of arrays."""
    n = d["ckg_e"].shape[0]
    w = dict(d)
    w["sk"] = np.stack([st.ternary_ntt(d["sk_bits"][0][k], d["sk_bits"][1][k]) for k in range(n)])
    w["u"] = np.stack([st.ternary_ntt(d["u_bits"][0][k], d["u_bits"][1][k]) for k in range(n)])
    sk, u, crp = w["sk"], w["u"], d["crp"]
    w["ckg"] = np.stack([st.ckg_share(sk[k], d["crs"], d["ckg_e"][k]) for k in range(n)])
    w["pk0"] = st.aggregate(list(w["ckg"]))
    w["r1"] = np.stack([st.rkg_round1(u[k], sk[k], crp, d["r1_e"][k]) for k in range(n)])
    w["r1_sum"] = st.aggregate(list(w["r1"]))
    w["r2"] = np.stack([st.rkg_round2(w["r1_sum"], sk[k], crp, d["r2_e"][k]) for k in range(n)])
    w["r2_sum"] = st.aggregate(list(w["r2"]))
    w["r3"] = np.stack([st.rkg_round3(w["r2_sum"], u[k], sk[k], d["r3_e"][k]) for k in range(n)])
    w["r3_sum"] = st.aggregate(list(w["r3"]))
    w["rlk"] = st.rkg_key(w["r2_sum"], w["r3_sum"])
    pk0, pk1 = w["pk0"], d["crs"]
    w["n1"] = np.stack([st.naive_round1(sk[k], pk0, pk1, d["n1_e"][k], d["n1_bits"][0][k], d["n1_bits"][1][k]) for k in range(n)])
    w["n1_sum"] = st.aggregate(list(w["n1"]))
    w["n2"] = np.stack([st.naive_round2(w["n1_sum"], sk[k], pk0, pk1, d["n2_bits"][0][k], d["n2_bits"][1][k], d["n2_e"][k]) for k in range(n)])
    w["n2_sum"] = st.aggregate(list(w["n2"]))
    w["rlk_naive"] = st.naive_key(w["n2_sum"])
    w["rtg"] = np.stack([np.stack([st.rtg_share(sk[k], g, d["crp_rot"][j], d["rtg_e"][j][k]) for k in range(n)]) for j, g in enumerate(gens)])
    w["rtg_sum"] = np.stack([st.aggregate(list(w["rtg"][j])) for j in range(len(gens))])
    w["rot"] = np.stack([st.rtg_key(w["rtg_sum"][j], d["crp_rot"][j]) for j in range(len(gens))])
    w["gens"] = list(gens)
    return w


CHAIN_PARAMS, CHAIN_SCALE, CHAIN_GEN = "PN12QP109", 2.0 ** 30, 5


def oracle_chain(oracle, N, Q, P, seed, roots):
    """three parties make a collective pk, rlk (three rounds) and one rotation key; then Encode -> Encrypt (pk, through P) -> MulRelin ->
    Rotate -> Decrypt under the sum of the secret keys, on the restatements and the oracle's plan with collective keys only.  Returns
    run_all's dict plus the plaintexts' inputs, the ciphertexts and the decrypted plaintext poly."""
    import ckks_encoder_ref as encoder_ref
    import ckks_encryptor_ref as encryptor_ref
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    st = Setup(oracle, N, Q, P, "ckks")
    w = run_all(st, inputs(N, Q, P, seed), [CHAIN_GEN])
    rng = np.random.default_rng(8000 + seed)
    cQ, level, slots = oracle.Context(N, Q), len(Q) - 1, N >> 1
    plan = oracle.CkksPlan(cQ, oracle.Context(N, P))
    coder, enc = encoder_ref.Encoder(oracle, N, Q, roots), encryptor_ref.Encryptor(oracle, N, Q, P)
    for k in ("x", "y"):
        w[k] = rng.uniform(0, 1, slots) * np.exp(2j * np.pi * rng.uniform(0, 1, slots))
        w[k + "_u"] = (draw(rng, (N >> 3,)), draw(rng, (N >> 3,)))
        w[k + "_e"] = (draw(rng, shape_noise=(N,)), draw(rng, shape_noise=(N,)))
    cts = [enc.encrypt_pk(False, level, w["pk0"], w["crs"], w[k + "_u"][0], w[k + "_u"][1], w[k + "_e"][0], w[k + "_e"][1],
                          coder.encode(w[k], level, CHAIN_SCALE)) for k in ("x", "y")]
    as_plan = lambda key: key.reshape(st.beta, 2, len(Q) + len(P), N)
    ct = plan.mulrelin(level, cts[0], cts[1], as_plan(w["rlk"]))
    ct = plan.permute_ntt(level, ct, CHAIN_GEN, as_plan(w["rot"][0]))
    w["sk_sum"] = st.aggregate(list(w["sk"]))
    w["pt"] = plan.decrypt(level, ct, w["sk_sum"][:level + 1])
    w["cts"] = cts
    return w
