"""lr_keygen on the device against the restatement over the CPU oracle (tests/keygen_ref.py), bit for bit: the secret key, the public key,
switching, relinearisation and rotation keys, host and device-pointer randomness, the default shape and lr_options::no_epilogue (the
reference's call-by-call shape), 1 and 3 keys per call, secret keys shared by the call or one per key, on
  n16        N = 2^4, 2 + 1 limbs of Qi60 / Pi60, beta 2: less than one workgroup, the 60-bit transform route
  PN12QP109  N = 2^12, 2 + 1 limbs, beta 2: CKKS moduli, the FP64-butterfly route
  PN13QP218  N = 2^13, 6 + 1 limbs, beta 6
  PN14QP438  its moduli at N = 2^11, 10 + 2 limbs, beta 5, alpha 2
  ragged     N = 2^11, the first 5 Q and both P of PN14QP438, beta 3: the last digit owns one row (the reference's break)
  n65536     N = 2^16, 2 + 1 limbs of PN16QP1761: one rotation key, one public key and one relinearisation key: the sub-block transform
             route, a 2^16 Galois gather, and the one degree at which a lane of the streaming kernels makes a second trip
The randomness carries every edge decision at fixed positions: the four ternary (coeff, sign) pairs, a bit plane of all ones, the noise
bytes (0, sign 0), (0, sign 1), (19, +-), (127, +-), with (0, sign 0) also on the last coefficient of another key; the uniform half has
coefficients 0 (q - MRed = q) and q_j - 1.  Galois elements 5, 5^-1, 2 N - 1, 1 and one element twice in a call; one and two powers of
sk.  Outputs are pre-filled with a pattern; the uniform halves and every input are compared unchanged afterwards.  The keys of one call
feed the key switch, the BFV relinearisation and the rotation; one chain runs on device-made keys only; every refusal of the header is
exercised; one _device call replays from a HIP graph.  70 keys in one call at n16 run the passes beyond the first 32 keys (rotation,
relinearisation with 70 powers, per-key secret keys); GenRotationKeysPow2 makes its whole set in one call."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import ckks_encoder_ref as encoder_ref
import keygen_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

K = 3
SHAPES = ["n16", "PN12QP109", "PN13QP218", "PN14QP438", "ragged"]
_CACHE = {}


def _moduli(pkg, name):
    if name == "n16":
        return 1 << 4, list(pkg.params.Qi60()[:2]), list(pkg.params.Pi60()[:1])
    if name == "n65536":
        N, Q, P = pkg.params.ckks_moduli("PN16QP1761")
        return N, list(Q[:2]), list(P[:1])
    if name == "ragged":
        _, Q, P = pkg.params.ckks_moduli("PN14QP438")
        return 1 << 11, list(Q[:5]), list(P)
    N, Q, P = pkg.params.ckks_moduli(name)
    return (1 << 11 if name == "PN14QP438" else N), list(Q), list(P)


def _case(oracle, pkg, name):
    """inputs of one shape and a cache of the restatement's keys: want(kind, ...) computes each once"""
    if name in _CACHE:
        return _CACHE[name]
    N, Q, P = _moduli(pkg, name)
    QP = Q + P
    rng = np.random.default_rng(len(name) * 1000 + N + 2)
    kg = ref.KeyGenerator(oracle, N, Q, P, "ckks")
    beta = kg.beta
    c = {"N": N, "Q": Q, "P": P, "beta": beta, "ref": kg}
    uc, us = ref.draw(rng, (K, N >> 3)), ref.draw(rng, (K, N >> 3))
    uc[0, 0], us[0, 0] = 0b10101010, 0b11001100          # coefficient i of byte 0: (coeff, sign) = (i & 1, (i >> 1) & 1)
    us[0, 1:] = 0xFF
    uc[1, :] = 0xFF                                        # a plane of all ones
    us[2, :] = 0xFF
    e, pk_e = ref.draw(rng, shape_noise=(K, beta, N)), ref.draw(rng, shape_noise=(K, N))
    for x in (e[:, 0], e[:, beta - 1], pk_e):
        x[0, :6] = [0, 0x80, 19, 19 | 0x80, 127, 127 | 0x80]
        x[1, N - 1] = 0                                    # (0, sign 0) on the last coefficient of another key
    a, pk1 = ref.uniform(rng, QP, N, K * beta).reshape(K, beta, len(QP), N), ref.uniform(rng, QP, N, K)
    for x in (a[0, 0], a[2, beta - 1], pk1[0]):
        x[:, 2] = 0                                        # a zero product: q - MRed = q
        x[:, N - 1] = np.array(QP, dtype=np.uint64) - np.uint64(1)
    c.update(uc=uc, us=us, e=e, pk_e=pk_e, a=a, pk1=pk1)
    c["sk"] = np.stack([kg.gen_secret_key(uc[b], us[b]) for b in range(K)])
    c["gens"] = [[5, pow(5, -1, 2 * N), 2 * N - 1], [1, 5, 5]]      # the identity gather, and one element twice in a call
    memo = {}

    def want(kind, k, *args):
        key = (kind, k) + args
        if key not in memo:
            sk = c["sk"]
            if kind == "pk":                    # args: index of the secret key
                memo[key] = kg.gen_public_key(sk[args[0]], pk_e[k], pk1[k])
            elif kind == "swk":                 # args: indices of skIn and skOut
                memo[key] = kg.gen_switching_key(sk[args[0]], sk[args[1]], e[k], a[k])
            elif kind == "rlk":                 # k = the power's index; sk[0]
                for i, x in enumerate(kg.gen_relin_keys(sk[0], 2, e[:2], a[:2])):
                    memo[("rlk", i)] = x
            else:                               # "rot": args: the Galois element; sk[0]
                memo[key] = kg.gen_rot_key(sk[0], args[0], e[k], a[k])
        return memo[key]
    c["want"] = want
    _CACHE[name] = c
    return c


def _bytes_on_device(ring, cQ, arrays):
    """byte arrays one behind the other in device memory (a one-limb poly used as a plain buffer); returns the poly and the pointers"""
    N = cQ.N
    flat = np.concatenate([np.ascontiguousarray(a, dtype=np.uint8).reshape(-1) for a in arrays])
    words = -(-flat.size // (8 * N)) * N
    buf = np.zeros(words * 8, dtype=np.uint8)
    buf[:flat.size] = flat
    poly = ring.Poly(cQ, 1, words // N).set(buf.view(np.uint64).reshape(words // N, 1, N))
    ptrs, off = [], 0
    for a in arrays:
        ptrs.append(poly.device_ptr + off)
        off += np.asarray(a).size
    return poly, ptrs


def _rings(ring, c, no_epilogue):
    opt = ring.Options(no_epilogue=1) if no_epilogue else ring.Options()
    return opt, ring.NewContextWithParams(c["N"], c["Q"], options=opt), ring.NewContextWithParams(c["N"], c["P"], options=opt)


def _pattern(batch, limbs, N):
    return (np.arange(batch * limbs * N, dtype=np.uint64) * np.uint64(2654435761) % np.uint64(1 << 30)).reshape(batch, limbs, N)


def _key_images(kg, c, n, first=0):
    """n key images: the pattern in the even members, the caller's uniform polys in the odd ones"""
    rows, beta, N = len(c["Q"]) + len(c["P"]), c["beta"], c["N"]
    out = []
    for k in range(first, first + n):
        img = _pattern(2 * beta, rows, N)
        img[1::2] = c["a"][k]
        out.append(kg.NewSwitchingKey().set(img))
    return out


def _check_keys(keys, wants, c, first, where):
    for k, (key, want) in enumerate(zip(keys, wants)):
        got = key.get()
        assert np.array_equal(got[0::2], want[0::2]), where + (k, "evakey[i][0]")
        assert np.array_equal(got[1::2], c["a"][first + k]), where + (k, "the uniform half changed")


@pytest.mark.parametrize("shared", [True, False], ids=["shared_keys", "own_keys"])
@pytest.mark.parametrize("n", [1, K])
@pytest.mark.parametrize("name", SHAPES)
def test_keys_against_the_restatement(gpu_pkg, oracle, name, n, shared):
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, name)
    N, rows, beta, want = c["N"], len(c["Q"]) + len(c["P"]), c["beta"], c["want"]
    kb = 1 if shared else n
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        kg = ring.KeyGenerator(cQ, cP, n, options=opt)
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x)
        rand = [c["uc"][:n], c["us"][:n], c["pk_e"][:n], c["e"][:n]]
        keep, ptrs = _bytes_on_device(ring, cQ, rand)
        for on_device in (False, True):
            where = (name, n, shared, no_epilogue, on_device)
            # the secret key
            sk = qp(_pattern(n, rows, N))
            if on_device:
                kg.GenSecretKeyDevice(ptrs[0:2], sk)
            else:
                kg.GenSecretKey(rand[0:2], sk)
            assert np.array_equal(sk.get().reshape(n, rows, N), c["sk"][:n]), where + ("sk",)
            # the public key: one secret key for the batch, or one each
            sk_in, pk = qp(c["sk"][:kb]), (qp(_pattern(n, rows, N)), qp(c["pk1"][:n]))
            if on_device:
                kg.GenPublicKeyDevice(sk_in, ptrs[2], pk)
            else:
                kg.GenPublicKey(sk_in, rand[2], pk)
            got = pk[0].get().reshape(n, rows, N)
            for b in range(n):
                assert np.array_equal(got[b], want("pk", b, 0 if shared else b)), where + ("pk0", b)
            assert np.array_equal(pk[1].get().reshape(n, rows, N), c["pk1"][:n]), where + ("pk1 changed",)
            # switching keys: skIn and skOut shared by the call (sk 0 -> sk 0 is a key too) or one per key (sk k -> sk (k + 1) % K)
            keys = _key_images(kg, c, n)
            sk_out = qp(c["sk"][:1]) if shared else qp(np.stack([c["sk"][(k + 1) % K] for k in range(n)]))
            if on_device:
                kg.GenSwitchingKeysDevice(sk_in, sk_out, ptrs[3], keys)
            else:
                kg.GenSwitchingKeys(sk_in, sk_out, rand[3], keys)
            _check_keys(keys, [want("swk", k, 0 if shared else k, 0 if shared else (k + 1) % K) for k in range(n)], c, 0, where + ("swk",))
            assert np.array_equal(sk_in.get().reshape(kb, rows, N), c["sk"][:kb]), where + ("skIn changed",)
            assert np.array_equal(sk_out.get().reshape(kb, rows, N)[0], c["sk"][0 if shared else 1]), where + ("skOut changed",)
            if shared:
                continue
            # relinearisation keys: one power (CKKS) or two (BFV, maxDegree = 2)
            sk0, powers = qp(c["sk"][:1]), min(n, 2)
            keys = _key_images(kg, c, powers)
            if on_device:
                kg.GenRelinKeysDevice(sk0, ptrs[3], keys)
            else:
                kg.GenRelinKeys(sk0, rand[3][:powers], keys)
            _check_keys(keys, [want("rlk", i) for i in range(powers)], c, 0, where + ("rlk",))
            # rotation keys
            for gens in ([g[:n] for g in c["gens"]] if n > 1 else [[5], [2 * N - 1]]):
                keys = _key_images(kg, c, n)
                if on_device:
                    kg.GenRotationKeysDevice(sk0, gens, ptrs[3], keys)
                else:
                    kg.GenRotationKeys(sk0, gens, rand[3], keys)
                _check_keys(keys, [want("rot", k, g) for k, g in enumerate(gens)], c, 0, where + ("rot", tuple(gens)))
            assert np.array_equal(sk0.get(), c["sk"][0]), where + ("sk changed",)
        del keep


def test_one_rotation_key_at_n65536(gpu_pkg, oracle):
    """the sub-block transform route and a 2^16 Galois gather, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n65536")
    rows, want = len(c["Q"]) + len(c["P"]), c["want"]("rot", 0, 5)
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        kg = ring.KeyGenerator(cQ, cP, 1, options=opt)
        sk = ring.Poly(cQ, rows, 1).set(c["sk"][:1])
        keys = _key_images(kg, c, 1)
        kg.GenRotationKeys(sk, [5], c["e"][:1], keys)
        _check_keys(keys, [want], c, 0, ("n65536", no_epilogue))


def test_public_and_relinearisation_key_at_n65536(gpu_pkg, oracle):
    """two trips of the streaming loops in the public key's pass and the powers of sk, in both shapes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n65536")
    N, rows, want = c["N"], len(c["Q"]) + len(c["P"]), c["want"]
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        kg = ring.KeyGenerator(cQ, cP, 1, options=opt)
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x)
        sk, pk = qp(c["sk"][:1]), (qp(_pattern(1, rows, N)), qp(c["pk1"][:1]))
        kg.GenPublicKey(sk, c["pk_e"][:1], pk)
        assert np.array_equal(pk[0].get().reshape(rows, N), want("pk", 0, 0)), no_epilogue
        keys = _key_images(kg, c, 1)
        kg.GenRelinKeys(sk, c["e"][:1], keys)
        _check_keys(keys, [want("rlk", 0)], c, 0, ("n65536", "rlk", no_epilogue))


MANY = 70      # more than the 32 keys of one pass: passes of 32, 32 and 6


def test_more_keys_than_one_pass(gpu_pkg, oracle):
    """n16 with max_batch = n_keys = 70: every offset a later pass adds -- into the bytes, the per-key secret keys, the Galois elements,
    the key array, the powers of sk -- and the pool's reuse across passes, in both shapes, host and device-pointer bytes"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P, beta, r = c["N"], c["Q"], c["P"], c["beta"], c["ref"]
    rows, rng = len(Q) + len(P), np.random.default_rng(4242)
    sk = np.stack([r.gen_secret_key(ref.draw(rng, (N >> 3,)), ref.draw(rng, (N >> 3,))) for _ in range(MANY)])
    e, a = ref.draw(rng, shape_noise=(MANY, beta, N)), ref.uniform(rng, Q + P, N, MANY * beta).reshape(MANY, beta, rows, N)
    cycle = [5, pow(5, -1, 2 * N), 2 * N - 1, 1, 25, 13, 7]
    gens = [cycle[k % len(cycle)] for k in range(MANY)]
    want = {"rot": [r.gen_rot_key(sk[0], gens[k], e[k], a[k]) for k in range(MANY)],
            "rlk": r.gen_relin_keys(sk[0], MANY, e, a),
            "swk": [r.gen_switching_key(sk[k], sk[(k + 1) % MANY], e[k], a[k]) for k in range(MANY)]}
    assert not np.array_equal(want["rlk"][33], want["rlk"][34]) and not np.array_equal(want["swk"][32], want["swk"][64])

    def images(kg):
        out = []
        for k in range(MANY):
            img = _pattern(2 * beta, rows, N)
            img[1::2] = a[k]
            out.append(kg.NewSwitchingKey().set(img))
        return out

    def check(keys, wants, where):
        for k in range(MANY):
            got = keys[k].get()
            assert np.array_equal(got[0::2], wants[k][0::2]), where + (k, "evakey[i][0]")
            assert np.array_equal(got[1::2], a[k]), where + (k, "the uniform half changed")
    for no_epilogue in (False, True):
        opt, cQ, cP = _rings(ring, c, no_epilogue)
        kg = ring.KeyGenerator(cQ, cP, MANY, options=opt)
        qp = lambda x: ring.Poly(cQ, rows, x.shape[0]).set(x)
        keep, ptrs = _bytes_on_device(ring, cQ, [e])
        sk0, sk_in, sk_out = qp(sk[:1]), qp(sk), qp(np.roll(sk, -1, axis=0))
        for on_device in (False, True):
            where = (no_epilogue, on_device)
            keys = images(kg)
            kg.GenRotationKeysDevice(sk0, gens, ptrs[0], keys) if on_device else kg.GenRotationKeys(sk0, gens, e, keys)
            check(keys, want["rot"], where + ("rot",))
            keys = images(kg)
            kg.GenRelinKeysDevice(sk0, ptrs[0], keys) if on_device else kg.GenRelinKeys(sk0, e, keys)
            check(keys, want["rlk"], where + ("rlk",))
            keys = images(kg)
            kg.GenSwitchingKeysDevice(sk_in, sk_out, ptrs[0], keys) if on_device else kg.GenSwitchingKeys(sk_in, sk_out, e, keys)
            check(keys, want["swk"], where + ("swk",))
        assert np.array_equal(sk_in.get(), sk) and np.array_equal(sk0.get(), sk[0])
        del keep


def test_rotation_keys_pow2_helper(gpu_pkg, oracle):
    """ring.KeyGenerator.GenRotationKeysPow2 at PN12QP109: its 2 (logN - 1) + 1 Galois elements are keygen_ref.pow2_galois_elements in
    GenRotationKeysPow2's order, and the whole set made in one call is the restatement's key by key"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "PN12QP109")
    N, Q, P, beta, r = c["N"], c["Q"], c["P"], c["beta"], c["ref"]
    rows = len(Q) + len(P)
    _, cQ, cP = _rings(ring, c, False)
    gens = r.pow2_galois_elements()
    n = len(gens)
    assert n == 2 * (12 - 1) + 1
    kg = ring.KeyGenerator(cQ, cP, n)
    assert kg.Pow2GaloisElements() == gens
    rng = np.random.default_rng(99)
    e, a = ref.draw(rng, shape_noise=(n, beta, N)), ref.uniform(rng, Q + P, N, n * beta).reshape(n, beta, rows, N)
    sk = ring.Poly(cQ, rows, 1).set(c["sk"][:1])
    got = kg.GenRotationKeysPow2(sk, e, a)
    assert sorted(got["left"]) == sorted(got["right"]) == [1 << i for i in range(11)]
    flat = []
    for i in range(11):
        flat += [got["left"][1 << i], got["right"][1 << i]]
    flat.append(got["conjugate"])
    assert [g for g, _ in flat] == gens and gens[-1] == 2 * N - 1
    for k, (g, key) in enumerate(flat):
        assert np.array_equal(key.get(), r.gen_rot_key(c["sk"][0], g, e[k], a[k])), (k, g)
    with pytest.raises(gpu_pkg._native.LatticeRingError):
        kg.GenRotationKeysPow2(sk, e, a[:-1])                  # the uniform halves are not optional


def test_secret_and_public_key_without_p(gpu_pkg, oracle):
    """ctxP == NULL is the reference's "modulus P is empty": the secret key and the public key over Q, the switching keys refused"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "n16")
    N, Q = c["N"], c["Q"]
    r = ref.KeyGenerator(oracle, N, Q, [], "ckks")
    cQ = ring.NewContextWithParams(N, Q)
    kg = ring.KeyGenerator(cQ, None, 1)
    sk = kg.GenSecretKey((c["uc"][:1], c["us"][:1]), kg.NewKey())
    want_sk = r.gen_secret_key(c["uc"][0], c["us"][0])
    assert np.array_equal(sk.get(), want_sk)
    pk1 = c["pk1"][0, :len(Q)]
    pk = kg.GenPublicKey(sk, c["pk_e"][:1], (kg.NewKey(), kg.NewKey().set(pk1)))
    assert np.array_equal(pk[0].get(), r.gen_public_key(want_sk, c["pk_e"][0], pk1))
    for call in (kg.NewSwitchingKey, lambda: kg.GenRelinKeys(sk, c["e"][:1], [sk])):       # the Python mirror refuses in the same words
        with pytest.raises(gpu_pkg._native.LatticeRingError, match="modulus P is empty") as e:
            call()
        assert e.value.code == 4
    with pytest.raises(gpu_pkg._native.LatticeRingError, match="modulus P is empty") as e:
        check = gpu_pkg._native.check
        check(gpu_pkg._native.lib().lr_keygen_relin_keys(kg.h, sk.h, 1, c["e"].ctypes.data_as(C.c_void_p), (C.c_void_p * 1)(sk.h.value)))
    assert e.value.code == 4


def test_staging_is_reused_across_consecutive_host_calls(gpu_pkg, oracle):
    """two host-form calls one behind the other with different bytes, no synchronisation between them: the second waits for the first
    one's copy out of the pinned buffer before it refills it"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "PN12QP109")
    rows = len(c["Q"]) + len(c["P"])
    _, cQ, cP = _rings(ring, c, False)
    kg = ring.KeyGenerator(cQ, cP, 1)
    sk = ring.Poly(cQ, rows, 1).set(c["sk"][:1])
    keys = [_key_images(kg, c, 1, first=k)[0] for k in range(2)]
    for k in range(2):
        kg.GenRotationKeys(sk, [5], c["e"][k:k + 1], [keys[k]])
    for k in range(2):
        _check_keys([keys[k]], [c["want"]("rot", k, 5)], c, k, ("staging", k))


def test_device_made_keys_feed_the_key_switch(gpu_pkg, oracle):
    """the keys of one call through lr_ckks_switch_keys, lr_bfv_relinearize and lr_ckks_rotate: the oracle plan's result, fed the
    restatement's keys"""
    ring = gpu_pkg.ring
    c = _case(oracle, gpu_pkg, "PN12QP109")
    N, Q, P, beta = c["N"], c["Q"], c["P"], c["beta"]
    nQ, rows, level = len(Q), len(Q) + len(P), len(Q) - 1
    _, cQ, cP = _rings(ring, c, False)
    kg, plan = ring.KeyGenerator(cQ, cP, K), ring.CkksPlan(cQ, cP, 1)
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    sk = ring.Poly(cQ, rows, 1).set(c["sk"][:1])
    gens = c["gens"][0]
    keys = kg.GenRotationKeys(sk, gens, c["e"], _key_images(kg, c, K))
    rlk = kg.GenRelinKeys(sk, c["e"][:1], _key_images(kg, c, 1))[0]
    as_plan = lambda key: key.reshape(beta, 2, rows, N)
    rng = np.random.default_rng(9)
    ct = ref.uniform(rng, Q, N, 3)
    dev = [cQ.NewPoly().set(x) for x in ct]
    p0, p1 = cQ.NewPoly(), cQ.NewPoly()
    plan.SwitchKeysInPlace(level, dev[2], rlk, p0, p1)
    w0, w1 = oplan.switch_keys(level, ct[2], as_plan(c["want"]("rlk", 0)))
    assert np.array_equal(p0.get(), w0) and np.array_equal(p1.get(), w1)
    out = (cQ.NewPoly(), cQ.NewPoly())
    plan.BfvRelinearize(dev, rlk, out)
    w = oplan.bfv_relinearize(ct, as_plan(c["want"]("rlk", 0)))
    assert np.array_equal(out[0].get(), w[0]) and np.array_equal(out[1].get(), w[1])
    for k, g in enumerate(gens):
        plan.PermuteNTT(level, dev[:2], g, keys[k], out)
        w = oplan.permute_ntt(level, ct[:2], g, as_plan(c["want"]("rot", k, g)))
        assert np.array_equal(out[0].get(), w[0]) and np.array_equal(out[1].get(), w[1]), g


def test_chain_on_device_made_keys_only(gpu_pkg, oracle):
    """secret -> public -> relinearisation and rotation key -> Encode -> Encrypt -> MulRelin -> Rescale -> Rotate -> Decrypt -> Decode on
    the device from the bytes of keygen_ref.chain_inputs: the decrypted plaintext poly equals the oracle chain's bit for bit, the slots
    are within keygen_ref.CHAIN_TOLERANCE of x * y rotated"""
    ring = gpu_pkg.ring
    N, Q, P = gpu_pkg.params.ckks_moduli(ref.CHAIN_PARAMS)
    Q, P = list(Q), list(P)
    level, slots, roots = len(Q) - 1, N >> 1, encoder_ref.roots_table(N)
    w = ref.oracle_chain(oracle, N, Q, P, 0, roots)
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    kg, plan, enc, coder = ring.KeyGenerator(cQ, cP, 1), ring.CkksPlan(cQ, cP, 1), ring.CkksEncryptor(cQ, cP, 1), ring.CkksEncoder(cQ, 1, roots)
    one = lambda x: np.asarray(x)[None]
    sk = kg.GenSecretKey((one(w["sk_bits"][0]), one(w["sk_bits"][1])), kg.NewKey())
    pk = kg.GenPublicKey(sk, one(w["pk_e"]), (kg.NewKey(), kg.NewKey().set(w["pk1"])))

    def image(a):
        img = np.zeros((2 * kg.beta, len(Q) + len(P), N), dtype=np.uint64)
        img[1::2] = a
        return kg.NewSwitchingKey().set(img)
    rlk = kg.GenRelinKeys(sk, w["rlk_e"], [image(w["rlk_a"][0])])[0]
    rot = kg.GenRotationKeys(sk, [w["gen"]], one(w["rot_e"]), [image(w["rot_a"])])[0]
    assert np.array_equal(sk.get(), w["sk"]) and np.array_equal(pk[0].get(), w["pk0"])
    assert np.array_equal(rlk.get(), w["rlk"]) and np.array_equal(rot.get(), w["rot"])
    cts = []
    for k in ("x", "y"):
        pt = coder.Encode(cQ.NewPoly(), one(w[k]), level, ref.CHAIN_SCALE)
        cts.append(enc.EncryptPk(pk, (one(w[k + "_u"][0]), one(w[k + "_u"][1])), (one(w[k + "_e"][0]), one(w[k + "_e"][1])), pt,
                                 (cQ.NewPoly(), cQ.NewPoly()), level, fast=False))
    ct = (cQ.NewPoly(), cQ.NewPoly())
    plan.MulRelin(level, cts[0], cts[1], rlk, ct)
    plan.Rescale(ct)
    out = (cQ.NewPoly(), cQ.NewPoly())
    plan.PermuteNTT(level - 1, ct, w["gen"], rot, out)
    pt = cQ.NewPoly()
    plan.Decrypt(level - 1, out, sk, pt)
    assert np.array_equal(pt.get()[:level], w["pt"])
    got = coder.Decode(pt, slots, level - 1, w["scale_out"]).reshape(slots)
    assert np.max(np.abs(got - w["slots_want"])) <= ref.CHAIN_TOLERANCE


def test_refusals(gpu_pkg, oracle):
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    c = _case(oracle, gpu_pkg, "n16")
    N, Q, P, beta = c["N"], c["Q"], c["P"], c["beta"]
    rows = len(Q) + len(P)
    cQ, cP, other = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, Q)

    def code(f, *args, **kw):
        with pytest.raises(nat.LatticeRingError) as e:
            f(*args, **kw)
        return e.value.code
    ARG, SHAPE = 4, 3
    # creation: as lr_ckks_encryptor_create
    assert code(ring.KeyGenerator, cQ, cP, 0) == ARG and code(ring.KeyGenerator, cQ, cP, 65536) == ARG                    # max_batch outside 1 .. 65535
    assert code(ring.KeyGenerator, ring.NewContextWithParams(4, Q), None, 1) == ARG                                       # N < 8
    assert code(ring.KeyGenerator, cQ, ring.NewContextWithParams(2 * N, P), 1) == ARG                                     # ctxP with another N
    if nat.device_count() > 1:
        assert code(ring.KeyGenerator, cQ, ring.NewContextWithParams(N, P, device=1), 1) == ARG                           # ctxP on another device
    L = nat.lib()
    assert L.lr_keygen_create(None, cP.h, 1, C.byref(C.c_void_p())) == ARG and L.lr_keygen_create(cQ.h, cP.h, 1, None) == ARG
    assert L.lr_keygen_destroy(None) == 0
    kg = ring.KeyGenerator(cQ, cP, 2)
    qp = lambda ctx, batch: ring.Poly(ctx, rows, batch)
    sk, sk2, pk = qp(cQ, 1), qp(cQ, 2), (qp(cQ, 2), qp(cQ, 2))
    bits, e2, e = (c["uc"][:2], c["us"][:2]), c["pk_e"][:2], c["e"][:2]
    keys = [kg.NewSwitchingKey(), kg.NewSwitchingKey()]
    # the secret key
    assert code(kg.GenSecretKey, bits, qp(other, 2)) == ARG                                                                # a poly of another context
    assert code(kg.GenSecretKey, bits, ring.Poly(cQ, rows - 1, 2)) == SHAPE                                                # too few limbs
    assert code(kg.GenSecretKey, (c["uc"], c["us"]), qp(cQ, 3)) == SHAPE                                                   # batch > max_batch
    # the public key
    assert code(kg.GenPublicKey, qp(other, 1), e2, pk) == ARG and code(kg.GenPublicKey, sk, e2, (pk[0], qp(other, 2))) == ARG
    assert code(kg.GenPublicKey, sk, e2, (qp(other, 2), pk[1])) == ARG
    assert code(kg.GenPublicKey, sk, e2, (pk[0], pk[0])) == ARG and code(kg.GenPublicKey, sk2, e2, (sk2, pk[1])) == ARG    # the output is an input
    assert code(kg.GenPublicKey, ring.Poly(cQ, rows - 1, 1), e2, pk) == SHAPE                                              # too few limbs
    assert code(kg.GenPublicKey, sk, e2, (pk[0], qp(cQ, 1))) == SHAPE                                                      # pk1 must have the batch
    assert code(kg.GenPublicKey, qp(cQ, 3), c["pk_e"], (qp(cQ, 3), qp(cQ, 3))) == SHAPE                                    # batch > max_batch
    # switching keys
    assert code(kg.GenSwitchingKeys, qp(other, 1), sk, e, keys) == ARG and code(kg.GenSwitchingKeys, sk, qp(other, 1), e, keys) == ARG
    assert code(kg.GenSwitchingKeys, sk, sk, e, [keys[0], ring.Poly(other, rows, 2 * beta)]) == ARG
    assert code(kg.GenSwitchingKeys, sk, sk, e, [keys[0], keys[0]]) == ARG                                                 # two outputs share memory
    inside = ring.Poly.wrap(cQ, keys[0].device_ptr, rows, 1)                                                               # member 0 of keys[0]
    assert code(kg.GenSwitchingKeys, inside, sk, e[:1], [keys[0]]) == ARG and code(kg.GenSwitchingKeys, sk, inside, e[:1], [keys[0]]) == ARG   # an output is an input
    assert code(kg.GenSwitchingKeys, sk, sk, e, [keys[0], ring.Poly(cQ, rows - 1, 2 * beta)]) == SHAPE                     # too few limbs
    assert code(kg.GenSwitchingKeys, sk, sk, e, [keys[0], ring.Poly(cQ, rows, 2 * beta + 1)]) == SHAPE                     # a key whose batch is not 2 beta
    assert code(kg.GenSwitchingKeys, sk, sk, e, [keys[0], ring.Poly(cQ, rows, 2 * beta - 1)]) == SHAPE
    assert code(kg.GenSwitchingKeys, qp(cQ, 3), sk, e, keys) == SHAPE                                                      # skIn has batch n_keys or 1
    assert code(kg.GenSwitchingKeys, sk, sk, c["e"], keys + [kg.NewSwitchingKey()]) == SHAPE                               # n_keys > max_batch
    assert code(kg.GenRelinKeys, sk, c["e"], keys + [kg.NewSwitchingKey()]) == SHAPE
    assert code(kg.GenRelinKeys, sk2, e, keys) == SHAPE                                                                    # one secret key
    assert code(kg.GenRotationKeys, sk, [5, 6], e, keys) == ARG and code(kg.GenRotationKeys, sk, [0, 5], e, keys) == ARG   # an even Galois element
    assert code(kg.GenRotationKeys, sk2, [5, 25], e, keys) == SHAPE
    # ctxQ and ctxP on different streams: every entry point of a handle with a ctxP refuses
    hip = C.CDLL("libamdhip64.so")
    st = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(st), 1) == 0                                                               # hipStreamNonBlocking
    cQ.SetStream(st.value)
    try:
        with pytest.raises(nat.LatticeRingError, match="different streams"):
            kg.GenSecretKey(bits, sk2)
        assert code(kg.GenSecretKeyDevice, (0x1000, 0x1000), sk2) == ARG and code(kg.GenPublicKey, sk, e2, pk) == ARG
        assert code(kg.GenSwitchingKeys, sk, sk, e, keys) == ARG and code(kg.GenRelinKeys, sk, e, keys) == ARG
        assert code(kg.GenRotationKeys, sk, [5, 25], e, keys) == ARG
    finally:
        cQ.Sync()
        cQ.SetStream(None)
        assert hip.hipStreamDestroy(st) == 0
    # raw calls: NULL arguments and counts < 1
    b = np.zeros(256, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    arr = (C.c_void_p * 2)(keys[0].h.value, keys[1].h.value)
    g2 = (C.c_uint64 * 2)(5, 25)
    h = lambda p: p.h
    calls = [("secret_key", [kg.h, b, b, 2, h(sk2)], 3), ("public_key", [kg.h, h(sk), b, 2, h(pk[0]), h(pk[1])], 3),
             ("switching_keys", [kg.h, h(sk), h(sk), b, 2, arr], 4), ("relin_keys", [kg.h, h(sk), 2, b, arr], 2),
             ("rotation_keys", [kg.h, h(sk), g2, 2, b, arr], 3)]
    for name, args, count in calls:
        for fn in (getattr(L, "lr_keygen_" + name), getattr(L, "lr_keygen_" + name + "_device")):
            for i in range(len(args)):
                if i != count:
                    assert fn(*[None if j == i else x for j, x in enumerate(args)]) == ARG, (fn.__name__, i)
            for bad in (0, -1):
                assert fn(*[bad if j == count else x for j, x in enumerate(args)]) == SHAPE, (fn.__name__, bad)
    assert L.lr_keygen_relin_keys(kg.h, h(sk), 2, b, (C.c_void_p * 2)(keys[0].h.value, None)) == ARG
    # the handle stays usable after its refusals
    sk.set(c["sk"][:1])
    keys = _key_images(kg, c, 2)
    kg.GenRotationKeys(sk, [5, 5], e, keys)
    _check_keys(keys, [c["want"]("rot", k, 5) for k in range(2)], c, 0, ("after the refusals",))


def test_device_form_replays_from_a_hip_graph(gpu_pkg):
    """tests/_keygen_graph_worker.py, in its own process because torch's HIP runtime has to come up before the library's"""
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_keygen_graph_worker.py")], cwd=ROOT, capture_output=True, text=True,
                         timeout=600)
    assert res.returncode == 0, res.stdout[-1500:] + res.stderr[-3000:]
    assert "graph replay ok" in res.stdout
