"""Test helper (not a test module): the key generators of ckks/keygen.go and bfv/keygen.go restated line by line over the CPU oracle's ring
primitives -- Context.ntt / ewise (MFORM, ADD, MUL_MONT, MUL_MONT_AND_ADD, MUL_MONT_AND_SUB, NEG, MUL_SCALAR_LIMBS) / permute_ntt -- one key
at a time, after the sampling.  The samplers' decisions arrive in the compact form of the encryptors and are expanded by
tests/bfv_encryptor_ref.py's rules; the uniform polys are arguments.  Polys are [|Q| + |P|, N] uint64 over contextQP, Q first, in NTT +
Montgomery form; a switching key is [2 beta, |Q| + |P|, N] with member 2 i = evakey[i][0] and member 2 i + 1 = evakey[i][1], the layout
the oracle's key switch reads.  Both Gaussian samplers are bound to contextQP (ckks/ckks.go:81, bfv/bfv.go:70)."""
import numpy as np

from bfv_encryptor_ref import expand_gaussian, expand_ternary

# The chain Encode -> Encrypt (pk) -> MulRelin -> Rescale -> Rotate -> Decrypt -> Decode of tests/test_oracle_keygen.py with generated keys
# only (PN12QP109, all slots, scale 2^30, seeds 0 .. 2): the largest slot error of the restatement over those runs, measured on the CPU,
# and what the tests allow -- 16 x that, the margin ROUND_TRIP_TOLERANCE of ckks_encryptor_ref.py uses, for the same reason (the spread
# of the sampler draws across seeds).
CHAIN_MEASURED = 2.689619e-03
CHAIN_TOLERANCE = 16 * CHAIN_MEASURED


class KeyGenerator:
    """NewKeyGenerator (ckks/keygen.go:79-94, bfv/keygen.go:70-84) for (N, Q, P); scheme = "ckks" or "bfv" selects whose lines run"""

    def __init__(self, oracle, N, Q, P, scheme="ckks"):
        assert scheme in ("ckks", "bfv")
        self.oracle, self.N, self.scheme = oracle, int(N), scheme
        self.Q, self.P = [int(q) for q in Q], [int(p) for p in P]
        self.moduli = self.Q + self.P
        self.ctx = oracle.Context(N, self.moduli)                                     # contextQP
        self.alpha = len(self.P)                                                      # params.Alpha()
        self.beta = -(-len(self.Q) // len(self.P)) if self.P else 0                   # params.Beta()
        self.Pbig = int(np.prod([int(p) for p in self.P], dtype=object)) if self.P else 1

    def mul_by_p(self, p):
        """Context.MulScalarBigint(p, contextP.ModulusBigint) (ring/ring.go:541-552)"""
        return self.ctx.ewise("MUL_SCALAR_LIMBS", p, scalars=[self.Pbig % q for q in self.moduli])

    def sample_ntt(self, e_bytes):
        """gaussianSampler.SampleNTTNew: Sample over contextQP, then Context.NTT"""
        return self.ctx.ntt(expand_gaussian(self.moduli, e_bytes, self.N))

    def gen_secret_key(self, coeff_bits, sign_bits):
        """GenSecretKey (ckks/keygen.go:97-106, bfv/keygen.go:87-96): SampleTernaryMontgomeryNTTNew"""
        return self.ctx.ntt(expand_ternary(self.oracle, self.moduli, coeff_bits, sign_bits, self.N))      # ckks :104, bfv :94

    def gen_public_key(self, sk, e_bytes, pk1):
        """GenPublicKey (ckks/keygen.go:138-151, bfv/keygen.go:121-136); pk1 = NewUniformPoly's draw"""
        pk0 = self.sample_ntt(e_bytes)                                                # ckks :144, bfv :129
        pk0 = self.ctx.ewise("MUL_MONT_AND_ADD", sk, pk1, out=pk0)                    # ckks :147, bfv :132
        return self.ctx.ewise("NEG", pk0)                                             # ckks :148, bfv :133

    def new_switching_key(self, skIn, skOut, e_bytes, a):
        """newSwitchingKey (ckks/keygen.go:282-338) / newswitchingkey (bfv/keygen.go:285-333); e_bytes [beta, N], a [beta, |QP|, N].
        The CKKS lines multiply skIn by P here (:290); the BFV callers have done it."""
        ctx, N = self.ctx, self.N
        skIn = np.array(skIn, dtype=np.uint64)
        if self.scheme == "ckks":
            skIn = self.mul_by_p(skIn)                                                # ckks :290
            last = len(self.Q) - 1                                                    # ckks :328 index >= levels - 1
        else:
            last = len(self.moduli) - 1                                               # bfv :322 index >= len(Modulus) - 1
        key = np.zeros((2 * self.beta, len(self.moduli), N), dtype=np.uint64)
        for i in range(self.beta):
            e = ctx.ewise("MFORM", self.sample_ntt(e_bytes[i]))                       # ckks :302-303, bfv :301-302
            key[2 * i + 1] = a[i]                                                     # ckks :306, bfv :304
            for j in range(self.alpha):                                               # ckks :315, bfv :309
                index = i * self.alpha + j
                row = ctx.ewise("ADD", _rows(e, index), _rows(skIn, index), level=index)      # ckks :323-325, bfv :317-319 (row `index` alone)
                e[index] = row[index]
                if index >= last:                                                     # ckks :328, bfv :322
                    break
            key[2 * i] = ctx.ewise("MUL_MONT_AND_SUB", key[2 * i + 1], skOut, out=e)  # ckks :334, bfv :329
        return key

    def gen_switching_key(self, skIn, skOut, e_bytes, a):
        """GenSwitchingKey (ckks/keygen.go:247-258, bfv/keygen.go:247-261)"""
        if self.scheme == "ckks":
            pool = np.array(skIn, dtype=np.uint64)                                    # :254 Copy
        else:
            pool = self.mul_by_p(skIn)                                                # bfv :255
        return self.new_switching_key(pool, skOut, e_bytes, a)                        # ckks :255, bfv :257

    def gen_relin_keys(self, sk, n_powers, e_bytes, a):
        """GenRelinKey: ckks/keygen.go:192-205 (n_powers = 1) and bfv/keygen.go:172-196 (n_powers = maxDegree); e_bytes [n_powers, beta, N].
        Key i switches from sk^(i + 2)."""
        ctx, keys = self.ctx, []
        if self.scheme == "ckks":
            pool = np.array(sk, dtype=np.uint64)                                      # :199
            for i in range(n_powers):                                                 # (the reference has one power: the loop restates it per key)
                pool = ctx.ewise("MUL_MONT", pool, sk)                                # :200
                keys.append(self.new_switching_key(pool, sk, e_bytes[i], a[i]))       # :201
        else:
            pool = self.mul_by_p(sk)                                                  # bfv :182-186
            for i in range(n_powers):                                                 # :188
                pool = ctx.ewise("MUL_MONT", pool, sk)                                # :189
                keys.append(self.new_switching_key(pool, sk, e_bytes[i], a[i]))       # :190
        return keys

    def gen_rot_key(self, sk, gen, e_bytes, a):
        """genrotKey (ckks/keygen.go:487-494) / genrotkey (bfv/keygen.go:429-441)"""
        pool = self.ctx.permute_ntt(sk, gen)                                          # ckks :489, bfv :433
        if self.scheme == "bfv":
            pool = self.mul_by_p(pool)                                                # bfv :435
        return self.new_switching_key(pool, sk, e_bytes, a)                           # ckks :490, bfv :437

    def pow2_galois_elements(self):
        """GenRotationKeysPow2 (ckks/keygen.go:391-417) in its order: left n, right n for n = 1, 2, .. < N / 2, then the conjugation"""
        N, mask = self.N, 2 * self.N - 1
        left, right, g, gi = [1], [1], 5, pow(5, 2 * N - 1, 2 * N)                    # ckks/ckks.go:83-85
        for _ in range(1, N >> 1):
            left.append(left[-1] * g & mask)
            right.append(right[-1] * gi & mask)
        out, n = [], 1
        while n < N >> 1:                                                             # :405
            out += [left[n], right[n]]                                                # :410-411
            n <<= 1
        return out + [2 * N - 1]                                                      # :415


def _rows(p, index):
    """limbs 0 .. index of a poly, for an ewise call whose result is read at row `index` only"""
    return np.ascontiguousarray(p[:index + 1])


def draw(rng, shape_planes=None, shape_noise=None):
    """sampler decisions from a numpy Generator: bit planes uint8 [..., N / 8] and / or noise bytes (magnitude below 20, any sign)"""
    if shape_planes is not None:
        return rng.integers(0, 256, shape_planes).astype(np.uint8)
    return (rng.integers(0, 20, shape_noise) | (rng.integers(0, 2, shape_noise) << 7)).astype(np.uint8)


def uniform(rng, moduli, N, batch=None):
    """NewUniformPoly's draw over the given moduli: [limbs, N], or [batch, limbs, N]"""
    one = lambda: np.array([rng.integers(0, int(q), N, dtype=np.uint64) for q in moduli], dtype=np.uint64)
    return one() if batch is None else np.stack([one() for _ in range(batch)])


CHAIN_PARAMS, CHAIN_SCALE, CHAIN_ROTATION = "PN12QP109", 2.0 ** 30, 1


def chain_inputs(N, Q, P, seed):
    """everything the chain draws, in one place, so that the device test feeds the same bytes"""
    rng = np.random.default_rng(1000 + seed)
    QP, beta, slots = list(Q) + list(P), -(-len(Q) // len(P)), N >> 1
    d = {"sk_bits": (draw(rng, (N >> 3,)), draw(rng, (N >> 3,))), "pk_e": draw(rng, shape_noise=(N,)), "pk1": uniform(rng, QP, N),
         "rlk_e": draw(rng, shape_noise=(1, beta, N)), "rlk_a": uniform(rng, QP, N, beta)[None],
         "rot_e": draw(rng, shape_noise=(beta, N)), "rot_a": uniform(rng, QP, N, beta)}
    for k in ("x", "y"):
        d[k] = rng.uniform(0, 1, slots) * np.exp(2j * np.pi * rng.uniform(0, 1, slots))
        d[k + "_u"] = (draw(rng, (N >> 3,)), draw(rng, (N >> 3,)))
        d[k + "_e"] = (draw(rng, shape_noise=(N,)), draw(rng, shape_noise=(N,)))
    return d


def oracle_chain(oracle, N, Q, P, seed, roots):
    """secret -> public -> relinearisation and rotation key -> Encode -> Encrypt (pk, through P) -> MulRelin -> Rescale -> Rotate by
    CHAIN_ROTATION -> Decrypt -> Decode, on the restatements and the oracle's plan with generated keys only.  Returns the inputs, every
    key, the decrypted plaintext poly and the decoded slots."""
    import ckks_encoder_ref as encoder_ref
    import ckks_encryptor_ref as encryptor_ref
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    d = chain_inputs(N, Q, P, seed)
    kg = KeyGenerator(oracle, N, Q, P, "ckks")
    cQ, level, slots = oracle.Context(N, Q), len(Q) - 1, N >> 1
    plan = oracle.CkksPlan(cQ, oracle.Context(N, P))
    coder, enc = encoder_ref.Encoder(oracle, N, Q, roots), encryptor_ref.Encryptor(oracle, N, Q, P)
    sk = kg.gen_secret_key(*d["sk_bits"])
    pk1 = d["pk1"]
    pk0 = kg.gen_public_key(sk, d["pk_e"], pk1)
    rlk = kg.gen_relin_keys(sk, 1, d["rlk_e"], d["rlk_a"])[0]
    gen = kg.pow2_galois_elements()[0] if CHAIN_ROTATION == 1 else pow(5, CHAIN_ROTATION, 2 * N)
    rot = kg.gen_rot_key(sk, gen, d["rot_e"], d["rot_a"])
    cts = [enc.encrypt_pk(False, level, pk0, pk1, d[k + "_u"][0], d[k + "_u"][1], d[k + "_e"][0], d[k + "_e"][1],
                          coder.encode(d[k], level, CHAIN_SCALE)) for k in ("x", "y")]
    as_plan = lambda key: key.reshape(kg.beta, 2, len(Q) + len(P), N)
    ct = plan.mulrelin(level, cts[0], cts[1], as_plan(rlk))
    ct = np.stack([cQ.rescale_op("oc_div_round_by_last_modulus_ntt", c) for c in ct])
    ct = plan.permute_ntt(level - 1, ct, gen, as_plan(rot))
    pt = plan.decrypt(level - 1, ct, sk[:level])
    scale = CHAIN_SCALE * CHAIN_SCALE / Q[level]
    got = coder.decode(pt, slots, level - 1, scale)
    want = np.roll(d["x"] * d["y"], -CHAIN_ROTATION)
    d.update(sk=sk, pk0=pk0, rlk=rlk, rot=rot, gen=gen, cts=cts, pt=pt, slots_out=got, slots_want=want, scale_out=scale)
    return d
