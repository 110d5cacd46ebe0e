"""lr_bfv_inner_sum and lr_bfv_rotate_chain (bfv.evaluator.InnerSum, bfv/evaluator.go:691-708, and rotateColumnsPow2, :637-666, as one
device call each) against tests/bfv_chain_ref.py -- the oracle's bfv_permute per step and (x + y) mod q per limb -- bit for bit: every BFV
parameter set, degrees on both sides of the fused route's bounds, N = 2 (the row step alone), batches, in place and out of place, a
different key per step, zeros that a negation turns into q; the same bits on every route; device-made keys end to end; the shape of the
reference's PIR example; every refusal of the header."""
import numpy as np
import pytest

import bfv_chain_ref as chain_ref

pytestmark = pytest.mark.gpu

T = 65537


def _moduli(pkg, name, small=False):
    _, Q, P, _ = pkg.params.bfv_moduli(name)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    return (Q[:2], P[:1]) if small else (Q, P)


def _inputs(pkg, Q, N, batch, seed):
    ct = [pkg.sampling.uniform_poly(Q, N, batch, seed=seed + k).reshape(batch, len(Q), N) for k in range(2)]
    ct[0][0, :, min(3, N - 1)] = 0      # a zero whose sign flips becomes q (ring_galois.go:121)
    ct[1][0, :, min(5, N - 1)] = 0
    return ct


def _host_keys(pkg, Q, P, N, count, seed):
    beta = -(-len(Q) // len(P))
    return [pkg.sampling.uniform_poly(Q + P, N, 2 * beta, seed=seed + i) for i in range(count)]


def _as_plan(key, Q, P, N):
    return key.reshape(-(-len(Q) // len(P)), 2, len(Q) + len(P), N)


def _device(pkg, Q, P, N, batch, keys_h, options=None):
    ring = pkg.ring
    if options is None:
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    else:
        cQ, cP = ring.NewContextWithParams(N, Q, options=options), ring.NewContextWithParams(N, P, options=options)
    plan = ring.CkksPlan(cQ, cP, batch, options=options)
    return cQ, plan, [plan.NewSwitchingKey().set(k) for k in keys_h]


def _up(cQ, ct, batch):
    return (cQ.NewPoly(batch).set(ct[0]), cQ.NewPoly(batch).set(ct[1]))


def _same(polys, want, where):
    for k in range(2):
        assert np.array_equal(polys[k].get().reshape(np.shape(want[k])), want[k]), where + (k,)


@pytest.mark.parametrize("name,small,logn,batch,no_pair", [
    ("PN13QP218", False, 11, 3, False), ("PN12QP109", False, 12, 1, False), ("PN12QP109", False, 12, 1, True), ("PN14QP438", False, 14, 1, False),
    ("PN13QP218", False, 13, 2, False), ("PN15QP880", True, 15, 1, False), ("PN15QP880", True, 10, 2, False),
    ("PN12QP109", True, 3, 2, False), ("PN12QP109", True, 2, 2, False), ("PN12QP109", True, 1, 2, False)])
def test_inner_sum_matches_the_composed_oracle(gpu_pkg, oracle, monkeypatch, name, small, logn, batch, no_pair):
    """InnerSum at every BFV set (PN14QP438 at full size: 14 steps), at N = 2^15 and 2^10 (one degree on each side of the fused route),
    and at N = 8, 4 and 2 (N = 2: no column step); out of place with the inputs left alone, and in place"""
    monkeypatch.delenv("LR_NO_PAIR", raising=False)
    if no_pair:
        monkeypatch.setenv("LR_NO_PAIR", "1")
    Q, P = _moduli(gpu_pkg, name, small)
    N = 1 << logn
    ct = _inputs(gpu_pkg, Q, N, batch, 300)
    keys_h = _host_keys(gpu_pkg, Q, P, N, logn, 400)      # logn - 1 column keys and the row key, every one different
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    plan_keys = [_as_plan(k, Q, P, N) for k in keys_h]
    want = [chain_ref.inner_sum(oplan, N, Q, np.stack([ct[0][b], ct[1][b]]), plan_keys[:-1], plan_keys[-1]) for b in range(batch)]
    want = [np.stack([w[k] for w in want]) for k in range(2)]
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    c, out = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.BfvInnerSum(c, keys[:-1], keys[-1], out)
    _same(out, want, (name, logn, "out of place"))
    _same(c, ct, (name, logn, "inputs"))
    plan.BfvInnerSum(c, keys[:-1], keys[-1], c)
    _same(c, want, (name, logn, "in place"))


@pytest.mark.parametrize("logn,batch", [(12, 2), (10, 2), (11, 1)])
def test_every_route_gives_the_same_bits(gpu_pkg, logn, batch):
    """the default plan, a plan with lr_options::no_epilogue and the step-by-step device composition (BfvPermute + Context.Add per step,
    what the overlay did before) at a degree on the fused route and one outside it, and for one ciphertext (the separate launches carry
    both components at once); accumulate and replace"""
    ring = gpu_pkg.ring
    Q, P = _moduli(gpu_pkg, "PN13QP218")
    N = 1 << logn
    ct = _inputs(gpu_pkg, Q, N, batch, 310)
    keys_h = _host_keys(gpu_pkg, Q, P, N, logn, 420)
    gens = chain_ref.inner_sum_elements(N)
    got = {}
    for route, opt in (("default", None), ("no_epilogue", ring.Options(no_epilogue=1))):
        cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h, opt)
        out = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.BfvInnerSum(_up(cQ, ct, batch), keys[:-1], keys[-1], out)
        rep = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.BfvRotateChain(_up(cQ, ct, batch), gens[:3], keys[:3], False, rep)
        got[route] = [p.get() for p in out + rep]
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    acc, tmp = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    for g, key in zip(gens, keys):
        plan.BfvPermute(acc, g, key, tmp)                  # RotateColumns / RotateRows (:702, :706)
        for k in range(2):
            cQ.Add(tmp[k], acc[k], acc[k])                 # evaluator.Add (:703, :707)
    rep = _up(cQ, ct, batch)
    for g, key in zip(gens[:3], keys[:3]):
        plan.BfvPermute(rep, g, key, rep)
    got["steps"] = [p.get() for p in acc + rep]
    for route in ("no_epilogue", "steps"):
        for k in range(4):
            assert np.array_equal(got["default"][k], got[route][k]), (logn, route, k)


@pytest.mark.parametrize("name,logn,batch", [("PN12QP109", 12, 2), ("PN12QP109", 10, 2), ("PN14QP438", 14, 1)])
def test_replace_chain_matches_the_oracle_and_the_host_loop(gpu_pkg, oracle, name, logn, batch):
    """rotateColumnsPow2 as one call: k = 5, k = N/2 - 1 (every bit set) and a right rotation (generator 5^-1 mod 2N), against the helper
    and against the BfvRotateColumnsPow2 host loop; n_steps = 0 copies.  On the fused route, below it, and for one ciphertext at
    N = 2^14 (2 + 1 limbs), the regime the route decision gives to the separate launches"""
    Q, P = _moduli(gpu_pkg, name, small=True)
    N = 1 << logn
    ct = _inputs(gpu_pkg, Q, N, batch, 320)
    keys_h = _host_keys(gpu_pkg, Q, P, N, logn - 1, 440)
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    pow2_h = {1 << i: _as_plan(k, Q, P, N) for i, k in enumerate(keys_h)}
    pow2 = {1 << i: k for i, k in enumerate(keys)}
    for generator, k in ((5, 5), (5, (N >> 1) - 1), (pow(5, -1, 2 * N), 6)):
        want = [chain_ref.rotate_columns_pow2(oplan, N, Q, np.stack([ct[0][b], ct[1][b]]), generator, k, pow2_h) for b in range(batch)]
        want = [np.stack([w[j] for w in want]) for j in range(2)]
        c, out, loop = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch)), (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.BfvRotateColumnsPow2Chain(c, generator, k, pow2, out)
        _same(out, want, (logn, generator, k, "out of place"))
        _same(c, ct, (logn, generator, k, "inputs"))
        plan.BfvRotateColumnsPow2(c, generator, k, pow2, loop)
        _same(loop, want, (logn, generator, k, "host loop"))
        plan.BfvRotateColumnsPow2Chain(c, generator, k, pow2, c)
        _same(c, want, (logn, generator, k, "in place"))
    c, out = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.BfvRotateChain(c, [], [], False, out)
    _same(out, ct, (logn, "no step"))
    plan.BfvRotateChain(c, [], [], True, (c[1], c[0]))                  # ... also into the other component's poly
    _same((c[1], c[0]), ct, (logn, "no step, crossed"))
    # one key handle for several steps, and an output over the other component's input
    gens = chain_ref.inner_sum_elements(N)[:2]
    want = [chain_ref.chain(oplan, Q, np.stack([ct[0][b], ct[1][b]]), gens, [pow2_h[1], pow2_h[1]], True) for b in range(batch)]
    c = _up(cQ, ct, batch)
    plan.BfvRotateChain(c, gens, [pow2[1], pow2[1]], True, (c[1], c[0]))
    _same((c[1], c[0]), [np.stack([w[j] for w in want]) for j in range(2)], (logn, "crossed"))


def _keygen(pkg, cQ, cP, rng):
    """lr_keygen: the secret key, the public key and GenRotationKeysPow2's whole set in one call"""
    ring = pkg.ring
    N, rows = cQ.N, len(cQ.Modulus) + len(cP.Modulus)
    moduli = [int(q) for q in cQ.Modulus] + [int(p) for p in cP.Modulus]
    n = 2 * (N.bit_length() - 2) + 1
    kg = ring.KeyGenerator(cQ, cP, n)
    bits = lambda b: rng.integers(0, 256, (b, N >> 3)).astype(np.uint8)
    noise = lambda *shape: (rng.integers(0, 20, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)
    uniform = lambda *lead: np.stack([rng.integers(0, q, lead + (N,), dtype=np.uint64) for q in moduli], axis=-2)
    sk = kg.GenSecretKey((bits(1), bits(1)), kg.NewKey())
    pk = kg.GenPublicKey(sk, noise(1, N), (kg.NewKey(), kg.NewKey().set(uniform(1))))
    rot = kg.GenRotationKeysPow2(sk, noise(n, kg.beta, N), uniform(n, kg.beta))
    col_keys = [rot["left"][1 << i][1] for i in range(N.bit_length() - 2)]
    return sk, pk, col_keys, rot["conjugate"][1], bits, noise


def test_inner_sum_end_to_end_on_device_made_keys(gpu_pkg):
    """PN12QP109: keys from lr_keygen, lr_bfv_encoder -> lr_bfv_encryptor -> lr_bfv_inner_sum -> decrypt -> decode: every slot holds the sum
    of the slots modulo t"""
    ring = gpu_pkg.ring
    N, Q, P, _ = gpu_pkg.params.bfv_moduli("PN12QP109")
    Q, P, batch = list(Q), list(P), 2
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    rng = np.random.default_rng(31)
    sk, pk, col_keys, row_key, bits, noise = _keygen(gpu_pkg, cQ, cP, rng)
    encoder, encryptor, decryptor = ring.BfvEncoder(cQ, T, batch), ring.BfvEncryptor(cQ, cP, batch), ring.BfvDecryptor(cQ, batch)
    plan = ring.CkksPlan(cQ, cP, batch)
    slots = rng.integers(0, T, size=(batch, N), dtype=np.uint64)
    ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    encryptor.EncryptPk(pk, (bits(batch), bits(batch)), (noise(batch, N), noise(batch, N)), encoder.EncodeUint(slots, cQ.NewPoly(batch)), ct)
    plan.BfvInnerSum(ct, col_keys, row_key, ct)
    got = encoder.DecodeUint(decryptor.Decrypt(ct, sk, cQ.NewPoly(batch)))
    want = np.array([int(s.astype(object).sum()) % T for s in slots], dtype=np.uint64)
    assert np.array_equal(got, np.broadcast_to(want[:, None], (batch, N)))


def test_pir_example_shape(gpu_pkg):
    """examples/dbfv/pir/pir.go:303-307 for a batch of 3 stored rows under shared keys: Mul(query, mask) (ciphertext x plaintext,
    lr_bfv_mul_deg), InnerSum, Mul(tmp, row) (lr_bfv_mul); decrypted and decoded, slot j of row b is (sum_i query_i mask_b,i) row_b,j mod t.
    PN13QP218's moduli at N = 2^11 leave room for the noise of two multiplications around 2^11 additions."""
    ring = gpu_pkg.ring
    _, Q, P, QMul = gpu_pkg.params.bfv_moduli("PN13QP218")
    Q, P, QMul, N, batch = list(Q), list(P), list(QMul), 1 << 11, 3
    cQ, cP, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, QMul)
    rng = np.random.default_rng(47)
    sk, pk, col_keys, row_key, bits, noise = _keygen(gpu_pkg, cQ, cP, rng)
    encoder, encryptor, decryptor = ring.BfvEncoder(cQ, T, batch), ring.BfvEncryptor(cQ, cP, batch), ring.BfvDecryptor(cQ, batch)
    mul, plan = ring.BfvPlan(cQ, cM, T, batch), ring.CkksPlan(cQ, cP, batch)
    query = np.zeros((batch, N), dtype=np.uint64)
    query[:, 77] = 1                                                     # pir.go:275-276, the same query for every row
    masks = rng.integers(0, T, size=(batch, N), dtype=np.uint64)
    rows = rng.integers(0, T, size=(batch, N), dtype=np.uint64)

    def encrypt(values):
        ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        return encryptor.EncryptPk(pk, (bits(batch), bits(batch)), (noise(batch, N), noise(batch, N)), encoder.EncodeUint(values, cQ.NewPoly(batch)), ct)
    enc_query, enc_rows = encrypt(query), encrypt(rows)
    tmp = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    mul.MulDeg(enc_query, (encoder.EncodeUint(masks, cQ.NewPoly(batch)),), tmp)      # :303
    plan.BfvInnerSum(tmp, col_keys, row_key, tmp)                                     # :305
    res = [cQ.NewPoly(batch) for _ in range(3)]
    mul.Mul(tmp, enc_rows, res)                                                       # :307
    got = encoder.DecodeUint(decryptor.Decrypt(res, sk, cQ.NewPoly(batch)))
    want = (masks[:, 77:78] * rows) % np.uint64(T)
    assert np.array_equal(got, want)


def test_refusals_leave_the_outputs_unwritten(gpu_pkg):
    """every refusal the header lists, with its code; argument checks come before shape checks; nothing is written"""
    ring, err = gpu_pkg.ring, gpu_pkg._native.LatticeRingError
    Q, P = _moduli(gpu_pkg, "PN13QP218")
    logn, nQ = 11, len(Q)
    N = 1 << logn
    keys_h = _host_keys(gpu_pkg, Q, P, N, 1, 460)
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, 1, keys_h)
    other, _, _ = _device(gpu_pkg, Q, P, N >> 1, 1, [])
    key = keys[0]
    cols = [key] * (logn - 1)
    mark = np.full((1, nQ, N), 7, dtype=np.uint64)
    c = (cQ.NewPoly(1).set(mark + 1), cQ.NewPoly(1).set(mark + 2))
    out = (cQ.NewPoly(1).set(mark), cQ.NewPoly(1).set(mark))
    big = [cQ.NewPoly(2) for _ in range(4)]
    narrow, short = cQ.NewPolyLvl(nQ - 2, 1), other.NewPoly(1)
    ARG, SHAPE = 4, 3

    def refused(code, call):
        with pytest.raises(err) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert all(np.array_equal(o.get().reshape(mark.shape), mark) for o in out)
    chain = lambda ct, gens, ks, o: plan.BfvRotateChain(ct, gens, ks, True, o)
    lib, h = gpu_pkg._native.lib(), lambda p: p.h
    refused(ARG, lambda: chain(c, [5, 25], [key, None], out))                                    # a null entry in keys
    refused(ARG, lambda: gpu_pkg._native.check(lib.lr_bfv_rotate_chain(plan.h, h(c[0]), h(c[1]), 1, None, None, 1, h(out[0]), h(out[1]))))
    refused(ARG, lambda: gpu_pkg._native.check(lib.lr_bfv_rotate_chain(plan.h, h(c[0]), None, 0, None, None, 1, h(out[0]), h(out[1]))))
    refused(ARG, lambda: gpu_pkg._native.check(lib.lr_bfv_rotate_chain(plan.h, h(c[0]), h(c[1]), -1, None, None, 1, h(out[0]), h(out[1]))))
    refused(ARG, lambda: chain(c, [5, 4], [key, key], out))                                      # an even Galois element
    refused(ARG, lambda: chain(c, [5], [key], (out[0], out[0])))                                 # the same output poly twice
    refused(ARG, lambda: chain((big[0], big[1]), [5], [key], (out[0], out[0])))                  # two reasons: the argument check comes first
    refused(SHAPE, lambda: chain((big[0], big[1]), [5], [key], (big[2], big[3])))                # a batch beyond max_batch
    refused(SHAPE, lambda: chain((c[0], narrow), [5], [key], out))                               # fewer limbs than Q
    refused(SHAPE, lambda: chain((short, c[1]), [5], [key], out))                                # another degree
    refused(SHAPE, lambda: chain(c, [5], [key], (out[0], big[0])))                               # another batch
    inner = lambda ct, ck, rk, o: plan.BfvInnerSum(ct, ck, rk, o)
    refused(ARG, lambda: inner(c, cols, None, out))                                              # no row key
    refused(ARG, lambda: inner(c, cols[:-1] + [None], key, out))                                 # a null entry in col_keys
    refused(ARG, lambda: inner(c, cols, key, (out[1], out[1])))
    refused(ARG, lambda: inner(c, cols[:-1], key, out))                                          # n_col_keys != log2(N) - 1
    refused(ARG, lambda: inner(c, cols + [key], key, out))
    refused(ARG, lambda: inner((big[0], big[1]), cols[:-1], key, (big[2], big[3])))              # wrong count and batch: the argument first
    refused(SHAPE, lambda: inner((big[0], big[1]), cols, key, (big[2], big[3])))
    refused(SHAPE, lambda: inner((narrow, c[1]), cols, key, out))
    refused(SHAPE, lambda: inner(c, cols, key, (short, out[1])))
    assert all(np.array_equal(c[k].get().reshape(mark.shape), mark + 1 + k) for k in range(2))
