"""lr_bfv_relinearize_deg (bfv.evaluator.Relinearize of every degree, bfv/evaluator.go:480-499, as one device call) against
tests/bfv_relin_ref.py -- the oracle's bfv_switch_keys per degree and a literal CRed per addition -- bit for bit: passes of four, of two
and one, and of one group throughout; full-size moduli; N = 2^15 and N = 8; out of place with the inputs left alone, then in place;
degree 2 against BfvRelinearize and degree 1 as a copy; the same bits on every route and for every max_batch, operands holding q and
2q - 1 included; device-made keys end to end through two multiplications; every refusal of the header."""
import numpy as np
import pytest

import bfv_relin_ref as relin_ref

pytestmark = pytest.mark.gpu

T = 65537


def _moduli(pkg, name, small=False):
    _, Q, P, _ = pkg.params.bfv_moduli(name)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    return (Q[:2], P[:1]) if small else (Q, P)


def _inputs(pkg, Q, N, batch, degree, seed):
    return [pkg.sampling.uniform_poly(Q, N, batch, seed=seed + k).reshape(batch, len(Q), N) for k in range(degree + 1)]


def _host_keys(pkg, Q, P, N, count, seed):
    beta = -(-len(Q) // len(P))
    return [pkg.sampling.uniform_poly(Q + P, N, 2 * beta, seed=seed + i) for i in range(count)]


def _as_plan(key, Q, P, N):
    return key.reshape(-(-len(Q) // len(P)), 2, len(Q) + len(P), N)


def _device(pkg, Q, P, N, max_batch, keys_h, options=None):
    ring = pkg.ring
    if options is None:
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    else:
        cQ, cP = ring.NewContextWithParams(N, Q, options=options), ring.NewContextWithParams(N, P, options=options)
    plan = ring.CkksPlan(cQ, cP, max_batch, options=options)
    return cQ, plan, [plan.NewSwitchingKey().set(k) for k in keys_h]


def _up(cQ, ct, batch):
    return [cQ.NewPoly(batch).set(x) for x in ct]


def _same(polys, want, where):
    for k, (p, w) in enumerate(zip(polys, want)):
        assert np.array_equal(p.get().reshape(np.shape(w)), w), where + (k,)


def _reference(oracle, Q, P, N, ct, keys_h, degree):
    """the helper per batch member: [2][batch, |Q|, N]"""
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    plan_keys = [_as_plan(k, Q, P, N) for k in keys_h]
    batch = ct[0].shape[0]
    per = [relin_ref.relinearize(oplan, Q, np.stack([c[b] for c in ct[:degree + 1]]), plan_keys) for b in range(batch)]
    return [np.stack([w[k] for w in per]) for k in range(2)]


@pytest.mark.parametrize("name,small,logn,batch,max_batch,degree", [
    ("PN12QP109", False, 12, 1, 4, 5),      # one pass of four groups; the single-ciphertext pair launches
    ("PN13QP218", False, 11, 2, 4, 4),      # passes of 2 and 1 groups: a partial last pass folding onto the outputs
    ("PN13QP218", False, 13, 3, 3, 3),      # G = 1 throughout
    ("PN14QP438", False, 14, 1, 8, 3),      # full-size moduli
    ("PN15QP880", True, 15, 1, 2, 3),       # the N = 2^15 transform routes at a merged batch of 2
    ("PN12QP109", True, 3, 2, 8, 5)])       # small-N HIP path
def test_relinearize_deg_matches_the_composed_oracle(gpu_pkg, oracle, name, small, logn, batch, max_batch, degree):
    """out of place with the inputs left alone, then in place; degree 2 on the same operands is BfvRelinearize; degree 1 copies"""
    Q, P = _moduli(gpu_pkg, name, small)
    N = 1 << logn
    ct = _inputs(gpu_pkg, Q, N, batch, degree, 600)
    keys_h = _host_keys(gpu_pkg, Q, P, N, degree - 1, 700)
    want = _reference(oracle, Q, P, N, ct, keys_h, degree)
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, max_batch, keys_h)
    c, out = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.BfvRelinearizeDeg(c, keys, out)
    _same(out, want, (name, logn, "out of place"))
    _same(c, ct, (name, logn, "inputs"))
    two, lin = (cQ.NewPoly(batch), cQ.NewPoly(batch)), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.BfvRelinearizeDeg(c[:3], keys[:1], two)
    plan.BfvRelinearize(c[:3], keys[0], lin)
    _same(two, [p.get() for p in lin], (name, logn, "degree 2"))
    plan.BfvRelinearizeDeg(c[:2], [], two)
    _same(two, ct[:2], (name, logn, "degree 1"))
    plan.BfvRelinearizeDeg(c, keys, (c[0], c[1]))
    _same(c[:2], want, (name, logn, "in place"))
    _same(c[2:], ct[2:], (name, logn, "inputs, in place"))


def _host_loop(cQ, plan, c, keys, batch):
    """what the overlay did before: per degree BfvSwitchKeys and two Context.Add"""
    acc = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    cQ.Copy(c[0], acc[0])
    cQ.Copy(c[1], acc[1])
    p = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    for deg in range(len(c) - 1, 1, -1):
        plan.BfvSwitchKeys(c[deg], keys[deg - 2], p[0], p[1])
        for k in range(2):
            cQ.Add(acc[k], p[k], acc[k])
    return acc


@pytest.mark.parametrize("logn,batch,degree,edge", [(11, 2, 5, False), (12, 1, 4, True), (10, 3, 3, False)])
def test_every_route_gives_the_same_bits(gpu_pkg, oracle, logn, batch, degree, edge):
    """the default plan at max_batch 1x, 2x and 4x the batch (G = 1, 2 and up to 4), a plan with lr_options::no_epilogue and the Python
    loop of BfvSwitchKeys + Context.Add; `edge`: ct[0] / ct[1] hold q and 2q - 1 in a few positions, where a sum that is reduced once at
    the end, or terms summed before the base, differ from the reference's chain of CRed -- also checked against the helper"""
    ring = gpu_pkg.ring
    Q, P = _moduli(gpu_pkg, "PN13QP218")
    N = 1 << logn
    ct = _inputs(gpu_pkg, Q, N, batch, degree, 620)
    if edge:
        q = np.array(Q, dtype=np.uint64)
        for k in range(2):
            ct[k][0, :, 1 + k] = q
            ct[k][0, :, 5 + k] = 2 * q - 1
            ct[k][batch - 1, :, N - 1 - k] = 2 * q - 1
    keys_h = _host_keys(gpu_pkg, Q, P, N, degree - 1, 720)
    got = {}
    for route, mult, opt in (("x1", 1, None), ("x2", 2, None), ("x4", 4, None), ("no_epilogue", 4, ring.Options(no_epilogue=1))):
        cQ, plan, keys = _device(gpu_pkg, Q, P, N, mult * batch, keys_h, opt)
        out = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.BfvRelinearizeDeg(_up(cQ, ct, batch), keys, out)
        got[route] = [p.get() for p in out]
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    got["loop"] = [p.get() for p in _host_loop(cQ, plan, _up(cQ, ct, batch), keys, batch)]
    for route in ("x2", "x4", "no_epilogue", "loop"):
        for k in range(2):
            assert np.array_equal(got["x1"][k], got[route][k]), (logn, route, k)
    if edge:
        want = _reference(oracle, Q, P, N, ct, keys_h, degree)
        for k in range(2):
            assert np.array_equal(got["x4"][k].reshape(want[k].shape), want[k]), (logn, "helper", k)


def test_degree_three_end_to_end_on_device_made_keys(gpu_pkg):
    """PN13QP218's moduli at N = 2^11 (the shape of test_pir_example_shape, room for two products): keys from lr_keygen with two powers,
    three encrypted slot vectors, Mul then MulDeg (2 x 1) to degree 3, lr_bfv_relinearize_deg, decrypt, decode: the slot-wise product
    modulo t -- and the degree-3 ciphertext decrypted as it is decodes to the same"""
    ring = gpu_pkg.ring
    _, Q, P, QMul = gpu_pkg.params.bfv_moduli("PN13QP218")
    Q, P, QMul, N, batch = list(Q), list(P), list(QMul), 1 << 11, 2
    cQ, cP, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P), ring.NewContextWithParams(N, QMul)
    rng = np.random.default_rng(53)
    moduli = [int(q) for q in Q] + [int(p) for p in P]
    kg = ring.KeyGenerator(cQ, cP, 2)
    bits = lambda b: rng.integers(0, 256, (b, N >> 3)).astype(np.uint8)
    noise = lambda *shape: (rng.integers(0, 20, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)
    uniform = lambda *lead: np.stack([rng.integers(0, q, lead + (N,), dtype=np.uint64) for q in moduli], axis=-2)
    sk = kg.GenSecretKey((bits(1), bits(1)), kg.NewKey())
    pk = kg.GenPublicKey(sk, noise(1, N), (kg.NewKey(), kg.NewKey().set(uniform(1))))

    def image():
        img = np.zeros((2 * kg.beta, len(moduli), N), dtype=np.uint64)
        img[1::2] = uniform(kg.beta)
        return kg.NewSwitchingKey().set(img)
    rlk = kg.GenRelinKeys(sk, noise(2, kg.beta, N), [image(), image()])          # the keys from s^2 and s^3 (bfv/keygen.go:172)
    encoder, encryptor, decryptor = ring.BfvEncoder(cQ, T, batch), ring.BfvEncryptor(cQ, cP, batch), ring.BfvDecryptor(cQ, batch)
    mul, plan = ring.BfvPlan(cQ, cM, T, batch), ring.CkksPlan(cQ, cP, 2 * batch)
    slots = [rng.integers(0, T, size=(batch, N), dtype=np.uint64) for _ in range(3)]

    def encrypt(values):
        ct = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        return encryptor.EncryptPk(pk, (bits(batch), bits(batch)), (noise(batch, N), noise(batch, N)), encoder.EncodeUint(values, cQ.NewPoly(batch)), ct)
    a, b, c = encrypt(slots[0]), encrypt(slots[1]), encrypt(slots[2])
    d2 = [cQ.NewPoly(batch) for _ in range(3)]
    mul.Mul(a, b, d2)
    d3 = [cQ.NewPoly(batch) for _ in range(4)]
    mul.MulDeg(d2, c, d3)
    want = (slots[0] * slots[1] % np.uint64(T)) * slots[2] % np.uint64(T)
    assert np.array_equal(encoder.DecodeUint(decryptor.Decrypt(d3, sk, cQ.NewPoly(batch))), want)
    lin = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.BfvRelinearizeDeg(d3, rlk, lin)
    assert np.array_equal(encoder.DecodeUint(decryptor.Decrypt(lin, sk, cQ.NewPoly(batch))), want)


def test_refusals_leave_everything_unwritten(gpu_pkg):
    """every refusal the header lists, with its code; argument checks come before shape checks; outputs and inputs are unwritten"""
    ring, err = gpu_pkg.ring, gpu_pkg._native.LatticeRingError
    Q, P = _moduli(gpu_pkg, "PN13QP218")
    N, nQ, nP = 1 << 11, len(Q), len(P)
    beta = -(-nQ // nP)
    keys_h = _host_keys(gpu_pkg, Q, P, N, 2, 760)
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, 1, keys_h)
    other, _, _ = _device(gpu_pkg, Q, P, N >> 1, 1, [])
    mark = np.full((1, nQ, N), 7, dtype=np.uint64)
    c = [cQ.NewPoly(1).set(mark + 1 + k) for k in range(4)]
    out = (cQ.NewPoly(1).set(mark), cQ.NewPoly(1).set(mark))
    big = [cQ.NewPoly(2) for _ in range(6)]
    narrow, short = cQ.NewPolyLvl(nQ - 2, 1), other.NewPoly(1)
    thin_key, short_key = ring.Poly(cQ, nQ + nP - 1, 2 * beta), ring.Poly(cQ, nQ + nP, 2 * beta - 1)
    ARG, SHAPE = 4, 3
    check, lib, h = gpu_pkg._native.check, gpu_pkg._native.lib(), lambda p: p.h

    def refused(code, call):
        with pytest.raises(err) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert all(np.array_equal(o.get().reshape(mark.shape), mark) for o in out)
    relin = lambda ct, ks, o: plan.BfvRelinearizeDeg(ct, ks, o)
    import ctypes as C
    table = lambda ps: (C.c_void_p * len(ps))(*[None if p is None else p.h.value for p in ps])
    raw = lambda pl, ct, degree, ks, o0, o1: check(lib.lr_bfv_relinearize_deg(pl, ct, degree, ks, o0, o1))
    refused(ARG, lambda: raw(None, table(c), 3, table(keys), h(out[0]), h(out[1])))              # null arguments
    refused(ARG, lambda: raw(plan.h, None, 3, table(keys), h(out[0]), h(out[1])))
    refused(ARG, lambda: raw(plan.h, table(c), 3, table(keys), None, h(out[1])))
    refused(ARG, lambda: raw(plan.h, table(c), 3, table(keys), h(out[0]), None))
    refused(ARG, lambda: raw(plan.h, table(c), 3, None, h(out[0]), h(out[1])))                    # degree >= 2 without keys
    refused(ARG, lambda: relin([c[0], c[1], None, c[3]], keys, out))                             # a null entry of ct
    refused(ARG, lambda: relin(c, [keys[0], None], out))                                         # a null entry of evks
    refused(ARG, lambda: raw(plan.h, table(c), 0, table(keys), h(out[0]), h(out[1])))            # a degree outside 1 .. 5
    refused(ARG, lambda: raw(plan.h, table(c + c), 6, table(keys * 3), h(out[0]), h(out[1])))
    refused(ARG, lambda: relin(c, keys, (out[0], out[0])))                                       # the same output poly twice
    refused(ARG, lambda: relin(c, keys, (c[2], out[1])))                                         # an output that is ct[k], k >= 2
    refused(ARG, lambda: relin(c, keys, (out[0], c[3])))
    refused(ARG, lambda: relin(c, keys, (c[1], out[1])))                                         # out0 being ct[1]
    refused(ARG, lambda: relin(c, keys, (out[0], c[0])))                                         # out1 being ct[0]
    refused(ARG, lambda: relin(big[:4], keys, (big[4], big[4])))                                 # two reasons: the argument check comes first
    refused(ARG, lambda: relin(c, [thin_key, keys[1]], (out[1], out[1])))
    refused(SHAPE, lambda: relin(big[:4], keys, (big[4], big[5])))                               # a batch beyond max_batch
    refused(SHAPE, lambda: relin([c[0], narrow, c[2], c[3]], keys, out))                         # fewer limbs than Q
    refused(SHAPE, lambda: relin([c[0], c[1], c[2], short], keys, out))                          # another ring degree
    refused(SHAPE, lambda: relin(c, keys, (out[0], big[0])))                                     # another batch
    refused(SHAPE, lambda: relin(c, keys, (narrow, out[1])))
    refused(SHAPE, lambda: relin(c, [keys[0], thin_key], out))                                   # a key image with fewer than |Q| + |P| limbs
    refused(SHAPE, lambda: relin(c, [short_key, keys[1]], out))                                  # ... with a batch below 2 beta
    assert all(np.array_equal(c[k].get().reshape(mark.shape), mark + 1 + k) for k in range(4))
