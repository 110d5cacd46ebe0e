"""Test helper (not a test module): the shapes and inputs of the seeded fuzz of the eight device handles (tests/test_gpu_handle_fuzz.py),
drawn without a device so that tests/test_handle_fuzz_shapes.py can check their coverage on the CPU.

draw(family, seed) is deterministic in (family, seed).  Moduli come from the two pools of tests/test_gpu_fuzz.py, which live here now:
_moduli (Qi60 / Pi60, generated 34-, 40- and 50-bit primes, the limit primes of tests/limit_moduli.py on both sides of 2^32, 2^33, 2^46,
2^57, 2^60 and below 2^61) and _ckks_size_moduli (30 .. 56 bits: contexts of the dual kernels).  Degrees run from the smallest one the
handle's header admits (N >= 8 for the handles that read bit planes of N / 8 bytes, N >= 2 for the two encoders) up to 2^13; the seeds
PINNED names run at 2^14 and 2^15 with |Q| <= 2, |P| = 1 and batch 1.  Nothing here is special-cased beyond those two seeds: the
coverage the CPU test asserts comes from the choice of BASE, the per-family offset of the seeds.

The inputs (noise bytes, bit planes, uniform polys, masks) are drawn by the helpers below from data_rng(d): the edge decisions -- noise
(0, sign 0), (0, sign 1), (19, +-), (127, +-), the ternary pairs, uniform coefficients 0 and q_j - 1, the refresh masks 0, +-1,
+-(2^64 - 1), +-2^64, the largest and smallest W-word values and multiples of a modulus -- sit at positions drawn per seed."""
import numpy as np

import limit_moduli as lm

FAMILIES = ("bfv_encoder", "ckks_encoder", "bfv_encryptor", "ckks_encryptor", "keygen", "collective", "refresh", "setup")
SEEDS = 12                               # the committed seeds of every family: 0 .. SEEDS - 1
PINNED = {10: 14, 11: 15}                # seed -> logN: the whole-limb assembly kernels behind the handles, |Q| <= 2, |P| = 1, batch 1
OPTION_SETS = {"default": {}, "no_epilogue": {"no_epilogue": 1}, "no_asm": {"no_asm": 1}}
BFV_T = (65537, 0x3ee0001)               # both = 1 mod 2^17: an NTT over Z_t exists at every degree drawn here
# the seeds' offset per family, chosen so that the committed seeds meet the coverage conditions of tests/test_handle_fuzz_shapes.py
BASE = {"bfv_encoder": 33, "ckks_encoder": 5, "bfv_encryptor": 32, "ckks_encryptor": 7, "keygen": 142, "collective": 23, "refresh": 389, "setup": 278}

MIN_LOGN = {"bfv_encoder": 1, "ckks_encoder": 1}                      # every other handle refuses N < 8
NO_P = ("bfv_encoder", "ckks_encoder")                                # handles over Q alone
EMPTY_P = ("bfv_encryptor", "ckks_encryptor", "keygen", "refresh", "setup")   # ctxP == NULL is admitted: the fast forms, sk and pk, CKKS, CKG
HAS_LEVEL = ("ckks_encoder", "ckks_encryptor", "collective", "refresh")
HAS_T = ("bfv_encoder", "refresh")


class _Params:
    """what the pool helpers read of the package: its params module (tests/limit_moduli.py loads the same file)"""
    params = lm.params


def _moduli(pkg, rng, logn, count):
    """a random mix of modulus sizes that are NTT-friendly for this degree"""
    pool = list(pkg.params.Qi60()[-8:]) + list(pkg.params.Pi60()[-4:])
    pool += pkg.params.GenerateNTTPrimes(40, logn, 3) + pkg.params.GenerateNTTPrimes(50, logn, 2) + pkg.params.GenerateNTTPrimes(34, logn, 1)
    # ... and the primes next to every admission bound (tests/limit_moduli.py)
    pool += [lm.below(61, logn), lm.above(60, logn), lm.below(60, logn), lm.above(57, logn), lm.below(57, logn), lm.above(46, logn), lm.below(46, logn),
             lm.above(33, logn), lm.below(33, logn), lm.above(32, logn), lm.below(32, logn)]
    pool = sorted(set(pool))
    idx = rng.choice(len(pool), size=count, replace=False)
    return [pool[i] for i in idx]


def _ckks_size_moduli(pkg, rng, logn, count):
    """moduli between 30 and 56 bits: contexts that select the dual assembly kernels (FP64 body below 2^46 next to the integer one)"""
    pool = []
    for bits in (30, 34, 40, 45, 46, 50, 56):
        pool += pkg.params.GenerateNTTPrimes(bits, logn, 2)
    # ... and the limit primes of that range (tests/limit_moduli.py): the top of the dual kernels' integer body, both sides of the FP64 body's
    # limit, both sides of 2^33 and 2^32 (FP64 limbs either way)
    pool += [lm.below(57, logn), lm.above(46, logn), lm.below(46, logn), lm.above(33, logn), lm.below(33, logn), lm.above(32, logn), lm.below(32, logn)]
    pool = sorted(set(pool))
    idx = rng.choice(len(pool), size=count, replace=False)
    return [pool[i] for i in idx]


def _level(rng, nq):
    """a level in 0 .. nq - 1: the two ends as often as everything between them"""
    kind = int(rng.integers(0, 4))
    return 0 if kind == 0 else nq - 1 if kind == 1 else int(rng.integers(0, nq))


def draw(family, seed):
    """the shape of one fuzz case; see the module docstring.  Every value is a Python int, str, bool, list or None."""
    assert family in FAMILIES
    rng = np.random.default_rng([FAMILIES.index(family), BASE[family], int(seed)])
    pinned = PINNED.get(int(seed))
    lo = MIN_LOGN.get(family, 3)
    if pinned is not None:
        logn = pinned
    else:
        band = int(rng.integers(0, 10))                               # 4 : 4 : 2 between the three bands of degrees
        logn = int(rng.integers(lo, 8)) if band < 4 else int(rng.integers(8, 12)) if band < 8 else int(rng.integers(12, 14))
    nq = int(rng.integers(1, 9))
    np_ = 0 if family in NO_P else int(rng.integers(1, 5))
    if family in EMPTY_P and int(rng.integers(0, 10)) == 0:
        np_ = 0
    batch = int(rng.integers(1, 6))
    if pinned is not None:
        nq, np_, batch = int(rng.integers(1, 3)), 0 if family in NO_P else 1, 1
    max_batch = batch + (int(rng.integers(1, 4)) if int(rng.integers(0, 2)) else 0)
    pool = _ckks_size_moduli if int(rng.integers(0, 4)) == 0 else _moduli
    mods = pool(_Params, rng, max(logn, 4), nq + np_)
    d = {"family": family, "seed": int(seed), "logn": logn, "Q": [int(q) for q in mods[:nq]], "P": [int(p) for p in mods[nq:]],
         "batch": batch, "max_batch": max_batch}
    d["level"] = _level(rng, nq) if family in HAS_LEVEL else nq - 1
    d["level_start"] = _level(rng, nq) if family == "refresh" else None
    d["t"] = int(BFV_T[int(rng.integers(0, 2))]) if family in HAS_T else None
    d["own_keys"] = bool(rng.integers(0, 2))                          # one key per batch member, or one shared by the call
    d["form"] = ("host", "device")[int(rng.integers(0, 2))]           # the randomness: host arrays, or pointers into device memory
    d["options"] = ("default", "no_epilogue", "no_asm")[int(rng.integers(0, 3))]
    d["options_on"] = ("context", "both")[int(rng.integers(0, 2))]    # on the contexts only (the handle inherits), or on the handle as well
    # per output, in the order the test makes them: None = a fresh poly, k = member k .. of a larger poly (Poly.wrap at an offset)
    d["out"] = [int(rng.integers(1, 3)) if int(rng.integers(0, 3)) == 0 else None for _ in range(4)]
    d["alias"] = bool(rng.integers(0, 2))                             # outputs alias operands where the header permits it
    d["scheme"] = ("ckks", "bfv")[int(rng.integers(0, 2))]           # whose lines the key generator's restatement runs (the same bits)
    d["expect_refusal"] = None
    if np_ == 0 and family in EMPTY_P:
        # the documented refusal of a handle without ctxP (LR_ERR_ARG = 4), asserted next to the entry points that do run
        d["expect_refusal"] = {"bfv_encryptor": "encrypt with fast = 0", "ckks_encryptor": "encrypt with fast = 0",
                               "keygen": "a switching-key entry point", "refresh": "a BFV entry point", "setup": "a P-protocol"}[family]
    if family == "ckks_encoder":
        top = logn - 1 if pinned is None else 6                       # the restatement's scale-up is a Python loop over 2 x slots coefficients
        d["slots"] = 1 << int(rng.integers(0, top + 1))
        d["logscale"] = (30, 40, 55)[int(rng.integers(0, 3))]
    if family == "bfv_encoder":
        d["n_values"] = (1 << logn) if int(rng.integers(0, 2)) else int(rng.integers(1, (1 << logn) + 1))
    if family in ("bfv_encryptor", "ckks_encryptor"):
        d["degree"] = int(rng.integers(1, 4))                         # of the ciphertext the decryptor gets
    if family in ("keygen", "setup"):
        N2 = 2 << logn
        picks = [1, N2 - 1, 5, pow(5, -1, N2)] + [int(rng.integers(0, N2 // 2)) * 2 + 1 for _ in range(4)]
        d["gens"] = [int(picks[int(rng.integers(0, len(picks)))]) for _ in range(batch)]
    if family in ("collective", "refresh", "setup"):
        d["n_shares"] = int(rng.integers(1, 5))                       # of the fold
    return d


def alpha_beta(d):
    nq, np_ = len(d["Q"]), len(d["P"])
    return np_, (-(-nq // np_) if np_ else 0)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def data_rng(d, stream=0):
    return np.random.default_rng([FAMILIES.index(d["family"]), BASE[d["family"]], d["seed"], 1 + stream])


NOISE_EDGES = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]


def noise(rng, shape):
    """noise bytes [..., N] of the regular sampler's range with the edge decisions at drawn positions of a drawn poly, and (0, sign 0) on the
    last coefficient of another"""
    e = (rng.integers(0, 20, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)
    flat = e.reshape(-1, e.shape[-1])
    N = flat.shape[1]
    pos = rng.choice(N, size=min(len(NOISE_EDGES), N), replace=False)
    flat[int(rng.integers(0, flat.shape[0])), pos] = NOISE_EDGES[:len(pos)]
    flat[int(rng.integers(0, flat.shape[0])), N - 1] = 0
    return e


def planes(rng, shape):
    """the two bit planes [..., N / 8] of a ternary poly: the four (coeff, sign) pairs in a drawn byte, a plane of all ones in a drawn poly"""
    c, s = rng.integers(0, 256, shape).astype(np.uint8), rng.integers(0, 256, shape).astype(np.uint8)
    fc, fs = c.reshape(-1, c.shape[-1]), s.reshape(-1, s.shape[-1])
    k, byte = int(rng.integers(0, fc.shape[0])), int(rng.integers(0, fc.shape[1]))
    fc[k, byte], fs[k, byte] = 0b10101010, 0b11001100
    (fc if rng.integers(0, 2) else fs)[int(rng.integers(0, fc.shape[0])), :] = 0xFF
    return c, s


def uniform(rng, moduli, N, batch):
    """uniform polys [batch, limbs, N] with coefficients 0 and q_j - 1 at drawn positions of a drawn member"""
    a = np.stack([np.array([rng.integers(0, int(q), N, dtype=np.uint64) for q in moduli], dtype=np.uint64) for _ in range(batch)])
    k, pos = int(rng.integers(0, batch)), rng.choice(N, size=2, replace=False)
    a[k, :, pos[0]] = 0
    a[k, :, pos[1]] = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    return a


def product(values):
    out = 1
    for v in values:
        out *= int(v)
    return out


def mask_words(Q, level_start):
    return -(-product(Q[:level_start + 1]).bit_length() // 64)


def refresh_masks(rng, Q, level_start, N):
    """N signed integers of W words: below Q_levelStart / 6 centred, as three parties draw them, with the edge values of
    tests/test_gpu_refresh.py's _edge_masks at drawn positions"""
    W = mask_words(Q, level_start)
    top = 1 << (64 * W - 1)
    edges = [v for v in (0, 1, -1, (1 << 64) - 1, -((1 << 64) - 1), 1 << 64, -(1 << 64), top - 1, -top, 3 * Q[0], -5 * Q[-1]) if -top <= v < top]
    bound = max(product(Q[:level_start + 1]) // 6, 1)
    nbytes = (bound.bit_length() + 7) // 8 + 8
    out = []
    for _ in range(N):
        v = int.from_bytes(rng.bytes(nbytes), "little") % bound
        out.append(v - bound if v >= bound >> 1 else v)
    pos = rng.choice(N, size=min(len(edges), N), replace=False)
    for p, v in zip(pos, edges):
        out[int(p)] = v
    return out


def recode_integers(rng, Q, level_start, N):
    """N integers in [0, Q_levelStart) for Recode to lift: both sides of Q_ls / 2 and the two ends at drawn positions"""
    Qls = product(Q[:level_start + 1])
    hand = [0, 1, (Qls - 1) // 2 - 1, (Qls - 1) // 2, (Qls + 1) // 2, Qls - 1]
    out = [int.from_bytes(rng.bytes(8 * len(Q) + 8), "little") % Qls for _ in range(N)]
    pos = rng.choice(N, size=min(len(hand), N), replace=False)
    for p, v in zip(pos, hand):
        out[int(p)] = v % Qls
    return out


# ---- the restatements' results for one shape ------------------------------------------------------------------------------------------------
def reference(oracle, d):
    """the inputs of the case and what the restatement (tests/*_ref.py) computes from them, each result once.  CPU only: the device test
    compares with it, the CPU test times it and checks its meaning with Python integers on the small seeds."""
    c = dict(d, N=1 << d["logn"], nQ=len(d["Q"]), nP=len(d["P"]), QP=d["Q"] + d["P"], rows=len(d["Q"]) + len(d["P"]))
    c["alpha"], c["beta"] = alpha_beta(d)
    c["n"] = d["batch"]
    c["kb"] = d["batch"] if d["own_keys"] else 1
    c["key"] = (lambda b: b) if d["own_keys"] else (lambda b: 0)
    return globals()["_ref_" + d["family"]](oracle, c, data_rng(d))


def _ref_bfv_encoder(oracle, c, rng):
    import bfv_encoder_ref
    N, Q, t, n, nv = c["N"], c["Q"], c["t"], c["n"], c["n_values"]
    r = c["ref"] = bfv_encoder_ref.Encoder(oracle, N, Q, t)
    u = rng.integers(0, 1 << 64, (n, nv), dtype=np.uint64)
    i = rng.integers(-(1 << 63), (1 << 63) - 1, (n, nv), dtype=np.int64)
    ue, ie = [0, t - 1, t, t + 1, (1 << 64) - 1], [-t, -1, 0, t >> 1, (t >> 1) + 1, -(1 << 63)]
    pos = rng.choice(nv, size=min(5, nv), replace=False)
    u[int(rng.integers(0, n)), pos] = np.array(ue[:len(pos)], dtype=np.uint64)
    i[int(rng.integers(0, n)), pos] = np.array(ie[:len(pos)], dtype=np.int64)
    c.update(u=u, i=i, pt=uniform(rng, Q, N, n))
    c["want_u"] = np.stack([r.encode_uint(u[b]) for b in range(n)])
    c["want_i"] = np.stack([r.encode_int(i[b]) for b in range(n)])
    c["dec_u"] = np.stack([r.decode_uint(c["pt"][b]) for b in range(n)])
    c["dec_i"] = np.stack([r.decode_int(c["pt"][b]) for b in range(n)])
    c["dec_back"] = np.stack([r.decode_uint(c["want_u"][b]) for b in range(n)])     # what was encoded, decoded again
    # floor(Q / t) m decodes to m exactly where the error m (Q mod t) / Q of the scaling stays below 1 / 2: Q > 2 t^2
    c["round_trip_exact"] = product(Q) > 2 * t * t
    return c


def _ref_ckks_encoder(oracle, c, rng):
    import ckks_encoder_ref
    N, Q, n, slots, level = c["N"], c["Q"], c["n"], c["slots"], c["level"]
    c["roots"] = ckks_encoder_ref.roots_table(N)
    r = c["ref"] = ckks_encoder_ref.Encoder(oracle, N, Q, c["roots"])
    c["scale"] = scale = 2.0 ** c["logscale"]
    v = rng.uniform(0, 1, (n, slots)) * np.exp(2j * np.pi * rng.uniform(0, 1, (n, slots)))
    k = int(rng.integers(0, n))
    v[k, ::3] = 0                                                     # zeros and exact halves among the slots of one member
    v[k, 1::5] = 0.5 - 0.25j
    c.update(values=v, pt=uniform(rng, Q[:level + 1], N, n))
    c["want_pt"] = [r.encode(v[b], level, scale) for b in range(n)]
    c["want_dec"] = [r.decode(c["want_pt"][b], slots, level, scale) for b in range(n)]
    c["want_dec_any"] = [r.decode(c["pt"][b], slots, level, scale) for b in range(n)]
    return c


def _encryptor_inputs(oracle, c, rng):
    import bfv_encryptor_ref
    N, Q, QP, n, kb = c["N"], c["Q"], c["QP"], c["n"], c["kb"]
    keys = [bfv_encryptor_ref.keygen(oracle, N, QP, rng)[:3] for _ in range(kb)]
    c["sk"], c["pk0"], c["pk1"] = (np.stack([k[i] for k in keys]) for i in range(3))
    c["pt"], c["crp"] = uniform(rng, Q, N, kb), uniform(rng, QP, N, n)
    (c["uc"], c["us"]), c["e0"], c["e1"], c["e"] = planes(rng, (n, N >> 3)), noise(rng, (n, N)), noise(rng, (n, N)), noise(rng, (n, N))
    c["forms"] = [(form, fast) for form in ("pk", "sk") for fast in ((True, False) if c["nP"] else (True,))]
    c["ct"] = [uniform(rng, Q, N, n) for _ in range(c["degree"] + 1)]  # the components a decryptor gets


def _ref_bfv_encryptor(oracle, c, rng):
    import bfv_encryptor_ref as ref
    _encryptor_inputs(oracle, c, rng)
    enc = c["ref"] = ref.Encryptor(oracle, c["N"], c["Q"], c["P"])
    key, want = c["key"], {}
    for form, fast in c["forms"]:
        if form == "pk":
            want[(form, fast)] = [enc.encrypt_pk(fast, c["pk0"][key(b)], c["pk1"][key(b)], c["uc"][b], c["us"][b], c["e0"][b], c["e1"][b],
                                                 c["pt"][key(b)]) for b in range(c["n"])]
        else:
            want[(form, fast)] = [enc.encrypt_sk(fast, c["sk"][key(b)], c["crp"][b], c["e"][b], c["pt"][key(b)]) for b in range(c["n"])]
    c["want"] = want
    c["want_dec"] = [ref.decrypt(enc.cQ, np.stack([x[b] for x in c["ct"]]), c["sk"][key(b)]) for b in range(c["n"])]
    return c


def _ref_ckks_encryptor(oracle, c, rng):
    import ckks_encryptor_ref as ref
    _encryptor_inputs(oracle, c, rng)
    enc = c["ref"] = ref.Encryptor(oracle, c["N"], c["Q"], c["P"])
    key, level, want = c["key"], c["level"], {}
    for form, fast in c["forms"]:
        if form == "pk":
            want[(form, fast)] = [enc.encrypt_pk(fast, level, c["pk0"][key(b)], c["pk1"][key(b)], c["uc"][b], c["us"][b], c["e0"][b],
                                                 c["e1"][b], c["pt"][key(b)]) for b in range(c["n"])]
        else:
            want[(form, fast)] = [enc.encrypt_sk(fast, level, c["sk"][key(b)], c["crp"][b], c["e"][b], c["pt"][key(b)]) for b in range(c["n"])]
    c["want"] = want
    return c


def _ref_keygen(oracle, c, rng):
    import keygen_ref as ref
    N, QP, n, beta, rows = c["N"], c["QP"], c["n"], c["beta"], c["rows"]
    kg = c["ref"] = ref.KeyGenerator(oracle, N, c["Q"], c["P"], c["scheme"])
    c["uc"], c["us"] = planes(rng, (n, N >> 3))
    c["sk"] = np.stack([kg.gen_secret_key(c["uc"][b], c["us"][b]) for b in range(n)])
    c["pk_e"], c["pk1"] = noise(rng, (n, N)), uniform(rng, QP, N, n)
    c["pk0"] = np.stack([kg.gen_public_key(c["sk"][c["key"](b)], c["pk_e"][b], c["pk1"][b]) for b in range(n)])
    if not c["nP"]:
        return c
    c["e"], c["a"] = noise(rng, (n, beta, N)), uniform(rng, QP, N, n * beta).reshape(n, beta, rows, N)
    c["sk_in"] = c["sk"][:c["kb"]]
    c["sk_out"] = np.roll(c["sk"], -1, axis=0) if c["own_keys"] else c["sk"][:1]       # own keys: sk k -> sk (k + 1) % n
    c["swk"] = [kg.gen_switching_key(c["sk_in"][c["key"](k)], c["sk_out"][c["key"](k)], c["e"][k], c["a"][k]) for k in range(n)]
    c["rlk"] = kg.gen_relin_keys(c["sk"][0], n, c["e"], c["a"])
    c["rot"] = [kg.gen_rot_key(c["sk"][0], c["gens"][k], c["e"][k], c["a"][k]) for k in range(n)]
    return c


def _secret_keys(oracle, c, rng, count):
    import keygen_ref
    kg = keygen_ref.KeyGenerator(oracle, c["N"], c["Q"], c["P"], "ckks")
    bits = [planes(rng, (c["N"] >> 3,)) for _ in range(count)]
    return kg, np.stack([kg.gen_secret_key(*b) for b in bits])


def _fold_inputs(c, rng, moduli, members, count):
    """`count` shares of `members` polys over `moduli` for a fold; two of them hold the residue q_j itself"""
    shares = [uniform(rng, moduli, c["N"], members) for _ in range(count)]
    q = np.array(moduli, dtype=np.uint64)
    shares[0][:, :, int(rng.integers(0, c["N"]))] = q
    shares[-1][:, :, int(rng.integers(0, c["N"]))] = q
    return shares


def _ref_collective(oracle, c, rng):
    import collective_ref as ref
    N, Q, QP, n, kb, nQ, level, key = c["N"], c["Q"], c["QP"], c["n"], c["kb"], c["nQ"], c["level"], c["key"]
    col = c["ref"] = ref.Collective(oracle, N, Q, c["P"])
    kg, sks = _secret_keys(oracle, c, rng, 3 * kb)
    c["sk_in"], c["sk_out"], tgt = sks[:kb], sks[kb:2 * kb].copy(), sks[2 * kb:]
    pos = int(rng.integers(0, N))
    c["sk_out"][0][:, pos] = c["sk_in"][0][:, pos]                    # Delta = CRed(q) = 0 on that coefficient
    c["pk1"] = uniform(rng, QP, N, kb)
    c["pk0"] = np.stack([kg.gen_public_key(tgt[b], noise(rng, (N,)), c["pk1"][b]) for b in range(kb)])
    c["c1"] = uniform(rng, Q, N, n)
    (c["uc"], c["us"]), c["e"] = planes(rng, (n, N >> 3)), noise(rng, (3, n, N))
    e = c["e"]
    c["ckks_cks"] = [col.ckks_cks_share(level, c["sk_in"][key(b)], c["sk_out"][key(b)], c["c1"][b], e[0, b]) for b in range(n)]
    c["bfv_cks"] = [col.bfv_cks_share(c["sk_in"][key(b)], c["sk_out"][key(b)], c["c1"][b], e[0, b]) for b in range(n)]
    pcks = lambda fn, *lead: [fn(*lead, c["sk_in"][key(b)], c["pk0"][key(b)], c["pk1"][key(b)], c["c1"][b], c["uc"][b], c["us"][b], e[1, b], e[2, b])
                              for b in range(n)]
    c["ckks_pcks"], c["bfv_pcks"] = pcks(col.ckks_pcks_share, level), pcks(col.bfv_pcks_share)
    c["shares"], c["base"] = _fold_inputs(c, rng, Q, n, c["n_shares"]), uniform(rng, Q, N, n)
    fold = lambda base: np.stack([col.aggregate([s[b, :level + 1] for s in c["shares"]], base[b] if base is not None else None) for b in range(n)])
    c["fold"], c["fold_base"] = fold(None), fold(c["base"])
    return c


def _ref_refresh(oracle, c, rng):
    import refresh_ref as ref
    N, Q, QP, n, kb, nQ, ls, key = c["N"], c["Q"], c["QP"], c["n"], c["kb"], c["nQ"], c["level_start"], c["key"]
    bfv = c["bfv"] = bool(c["nP"])
    r = c["ref"] = ref.Refresh(oracle, N, Q, c["P"], c["t"] if bfv else 0)
    _, c["sk"] = _secret_keys(oracle, c, rng, kb)                     # over Q||P; the CKKS calls read the rows of Q
    c["c1"], c["crs"], c["c0"] = uniform(rng, Q, N, n), uniform(rng, Q, N, n), uniform(rng, Q, N, n)
    c["dec"], c["rec"] = uniform(rng, Q, N, n), uniform(rng, Q, N, n)  # what a fold of shares may hold
    c["e"] = noise(rng, (2, n, N))
    c["words"] = mask_words(Q, ls)
    c["mask"] = [refresh_masks(rng, Q, ls, N) for _ in range(n)]
    c["ckks_shares"] = [r.ckks_gen_shares(ls, c["sk"][key(b)][:nQ], c["c1"][b], c["crs"][b], c["mask"][b], c["e"][0, b], c["e"][1, b]) for b in range(n)]
    # the sums c0 + dec that Recode lifts carry the hand-set integers; c0 is chosen to produce them
    c["sum"] = np.stack([r.cQ.ntt(r.set_coefficients_bigint(recode_integers(rng, Q, ls, N), ls + 1)) for _ in range(n)])
    c["c0_at"] = np.stack([r.cQ.ewise("SUB", c["sum"][b], c["dec"][b][:ls + 1]) for b in range(n)])
    c["recode"] = [r.ckks_recode(c["sum"][b]) for b in range(n)]
    c["ckks_finalize"] = [r.ckks_finalize(ls, c["c0_at"][b], c["dec"][b], c["rec"][b]) for b in range(n)]
    if bfv:
        c["crs_qp"] = uniform(rng, QP, N, n)
        m = rng.integers(0, c["t"], (n, N)).astype(np.uint64)
        m[int(rng.integers(0, n)), rng.choice(N, size=2, replace=False)] = [0, c["t"] - 1]
        c["mask_bfv"] = m
        c["bfv_shares"] = [r.bfv_gen_shares(c["sk"][key(b)], c["c1"][b], c["crs_qp"][b], m[b], c["e"][0, b], c["e"][1, b]) for b in range(n)]
        c["bfv_finalize"] = [r.bfv_finalize(c["c0"][b], c["crs_qp"][b], c["dec"][b], c["rec"][b]) for b in range(n)]
    c["shares"] = _fold_inputs(c, rng, Q, n, c["n_shares"])
    c["fold"] = np.stack([r.aggregate([s[b, :c["level"] + 1] for s in c["shares"]]) for b in range(n)])
    return c


def _ref_setup(oracle, c, rng):
    import setup_ref as ref
    N, Q, P, QP, n, kb, beta, rows, key = c["N"], c["Q"], c["P"], c["QP"], c["n"], c["kb"], c["beta"], c["rows"], c["key"]
    st, ck = ref.Setup(oracle, N, Q, P, "bfv"), ref.Setup(oracle, N, Q, P, "ckks")
    c["ref"] = st
    bits = lambda *shape: planes(rng, shape + (N >> 3,))
    sb, ub = bits(kb), bits(kb)
    c["sk"] = np.stack([st.ternary_ntt(sb[0][k], sb[1][k]) for k in range(kb)])
    c["u"] = np.stack([st.ternary_ntt(ub[0][k], ub[1][k]) for k in range(kb)])
    c["crs"], c["ckg_e"] = uniform(rng, QP, N, 1)[0], noise(rng, (n, N))
    sk, u = (lambda k: c["sk"][key(k)]), (lambda k: c["u"][key(k)])
    w = c["want"] = {"ckg": [st.ckg_share(sk(k), c["crs"], c["ckg_e"][k]) for k in range(n)]}
    members = (1, beta, 2 * beta)[int(rng.integers(0, 3))] if P else 1
    c["shares"] = _fold_inputs(c, rng, QP, members, c["n_shares"])
    w["fold"] = st.aggregate([s[0] if members == 1 else s for s in c["shares"]])
    if not P:
        return c
    c["crp"] = uniform(rng, QP, N, beta)
    # the aggregates a later round reads are inputs of that round: uniform polys serve
    for k, m in (("pk0", 1), ("r1_sum", beta), ("r2_sum", 2 * beta), ("r3_sum", beta), ("n1_sum", 2 * beta), ("n2_sum", 2 * beta)):
        c[k] = uniform(rng, QP, N, m)
    c["pk0"] = c["pk0"][0]
    c["r1_e"], c["r2_e"], c["r3_e"] = noise(rng, (n, beta, N)), noise(rng, (n, beta, 2, N)), noise(rng, (n, beta, N))
    c["n1_e"], c["n2_e"], c["rtg_e"] = noise(rng, (n, beta, 2, N)), noise(rng, (n, beta, 2, N)), noise(rng, (n, beta, N))
    c["n1_bits"], c["n2_bits"] = bits(n, beta), bits(n, beta)
    crp, pk0, pk1 = c["crp"], c["pk0"], c["crs"]
    w["r1"] = [st.rkg_round1(u(k), sk(k), crp, c["r1_e"][k]) for k in range(n)]
    w["r2"] = [st.rkg_round2(c["r1_sum"], sk(k), crp, c["r2_e"][k]) for k in range(n)]
    w["r3"] = [st.rkg_round3(c["r2_sum"], u(k), sk(k), c["r3_e"][k]) for k in range(n)]
    for name, s in (("n1_bfv", st), ("n1_ckks", ck)):
        w[name] = [s.naive_round1(sk(k), pk0, pk1, c["n1_e"][k], c["n1_bits"][0][k], c["n1_bits"][1][k]) for k in range(n)]
    w["n2"] = [st.naive_round2(c["n1_sum"], sk(k), pk0, pk1, c["n2_bits"][0][k], c["n2_bits"][1][k], c["n2_e"][k]) for k in range(n)]
    w["rtg"] = [st.rtg_share(c["sk"][0], c["gens"][k], crp, c["rtg_e"][k]) for k in range(n)]
    w["rlk"], w["rlk_naive"], w["rot"] = st.rkg_key(c["r2_sum"], c["r3_sum"]), st.naive_key(c["n2_sum"]), st.rtg_key(c["r1_sum"], crp)
    return c
