"""lr_ckks_rotate_chain (rotateColumnsPow2, ckks/evaluator.go:1402-1424, and the slot-sum loop RotateColumns; Add as one device call)
against tests/ckks_chain_ref.py -- the oracle's permute_ntt per step and (r + a) mod q per limb -- bit for bit: the assembly transforms of
N = 2^15 and 2^16, polys with more limbs than level + 1, small rings off the fused route, batches, in place and out of place, a different
key per step, planted zeros and q - 1; the same bits on every route; the RotateColumnsPow2 host loop; device-made keys end to end; every
refusal of the header."""
import numpy as np
import pytest

import ckks_chain_ref as chain_ref

pytestmark = pytest.mark.gpu


def _moduli(pkg, name, cut):
    _, Q, P = pkg.params.ckks_moduli(name)
    Q, P = [int(q) for q in Q], [int(p) for p in P]
    return (Q[:2], P[:1]) if cut else (Q, P)


def _inputs(pkg, Q, N, batch, seed):
    """uniform polys over all of Q with a few zeros and q - 1 planted"""
    ct = [pkg.sampling.uniform_poly(Q, N, batch, seed=seed + k).reshape(batch, len(Q), N) for k in range(2)]
    top = np.array(Q, dtype=np.uint64) - 1
    ct[0][0, :, min(3, N - 1)] = 0
    ct[1][0, :, min(5, N - 1)] = 0
    ct[0][-1, :, N - 1] = top
    ct[1][-1, :, 0] = top
    ct[0][0, :, 1] = top      # ... and a pair that a step adds: q - 1 and its image
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
    """polys over all of Q, whatever the level of the call: their stride is |Q| N"""
    return (cQ.NewPoly(batch).set(ct[0]), cQ.NewPoly(batch).set(ct[1]))


def _same(polys, want, level, where):
    for k in range(2):
        got = polys[k].get().reshape(np.shape(want[k]))
        assert np.array_equal(got[:, :level + 1], want[k][:, :level + 1]), where + (k,)


def _want(oplan, level, Q, ct, batch, gens, keys, accumulate):
    """the helper's chain per batch member, as [2][batch, |Q|, N] with the limbs above `level` left as the inputs have them"""
    out = [np.array(ct[0]), np.array(ct[1])]
    for b in range(batch):
        w = chain_ref.chain(oplan, level, Q, np.stack([ct[0][b, :level + 1], ct[1][b, :level + 1]]), gens, keys, accumulate)
        for k in range(2):
            out[k][b, :level + 1] = w[k]
    return out


CASES = [
    # name, moduli cut to Q[:2] P[:1], log2(N), batch, level (None: the top)
    ("PN15QP880", True, 15, 1, None),        # assembly transforms, sub-block split
    ("PN15QP880", True, 15, 2, None),
    ("PN16QP1761", True, 16, 1, None),       # the top stage inside the extensions, forked launches
    ("PN12QP109", False, 12, 3, 0),          # level 0 is also one below the top: the polys have more limbs than level + 1
    ("PN12QP109", False, 12, 3, None),
    ("PN15QP880", True, 10, 2, None),        # no transform epilogue: the composed route
    ("PN15QP880", True, 3, 2, None),
    ("PN15QP880", True, 2, 2, None),
]


@pytest.mark.parametrize("name,cut,logn,batch,level", CASES)
def test_chain_matches_the_composed_oracle(gpu_pkg, oracle, name, cut, logn, batch, level):
    """replacing with k = 5, k = n/2 - 1 (every bit set) and a right rotation, also against the RotateColumnsPow2 host loop, and the
    accumulating chain over the whole slot sum; out of place with the inputs left alone, and in place; every step under its own key"""
    Q, P = _moduli(gpu_pkg, name, cut)
    N = 1 << logn
    level = len(Q) - 1 if level is None else level
    ct = _inputs(gpu_pkg, Q, N, batch, 300)
    nkeys = max(logn - 1, 3)
    keys_h = _host_keys(gpu_pkg, Q, P, N, nkeys, 400)
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    pow2_h = {1 << i: _as_plan(k, Q, P, N) for i, k in enumerate(keys_h)}
    for left, k in ((True, 5), (True, max((N >> 1) - 1, 1)), (False, 6)):
        steps = chain_ref.pow2_steps(N, k, left)
        want = _want(oplan, level, Q, ct, batch, [g for g, _ in steps], [pow2_h[i] for _, i in steps], False)
        pow2 = {1 << i: (pow(5, (1 << i) if left else -(1 << i), 2 * N), key) for i, key in enumerate(keys)}
        c, out, loop = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch)), (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.RotateColumnsPow2Chain(level, c, k, pow2, out)
        _same(out, want, level, (logn, left, k, "out of place"))
        _same(c, ct, len(Q) - 1, (logn, left, k, "inputs"))
        plan.RotateColumnsPow2(level, c, k, pow2, loop)
        _same(loop, want, level, (logn, left, k, "host loop"))
        plan.RotateColumnsPow2Chain(level, c, k, pow2, c)
        _same(c, want, level, (logn, left, k, "in place"))
    gens = chain_ref.slot_sum_elements(N)
    want = _want(oplan, level, Q, ct, batch, gens, [pow2_h[1 << i] for i in range(len(gens))], True)
    c, out = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.RotateChain(level, c, gens, keys[:len(gens)], True, out)
    _same(out, want, level, (logn, "slot sum, out of place"))
    _same(c, ct, len(Q) - 1, (logn, "slot sum, inputs"))
    plan.RotateChain(level, c, gens, keys[:len(gens)], True, c)
    _same(c, want, level, (logn, "slot sum, in place"))
    if level < len(Q) - 1:
        for k in range(2):      # the limbs above the level are nobody's to write
            assert np.array_equal(c[k].get().reshape(ct[k].shape)[:, level + 1:], ct[k][:, level + 1:]), (logn, "above the level", k)


@pytest.mark.parametrize("name,logn,batch", [("PN12QP109", 12, 2), ("PN15QP880", 15, 1)])
def test_every_route_gives_the_same_bits(gpu_pkg, name, logn, batch):
    """the default plan, a plan with lr_options::no_epilogue and the step-by-step device composition (PermuteNTT + Context.Add per step);
    accumulate and replace"""
    ring = gpu_pkg.ring
    Q, P = _moduli(gpu_pkg, name, name != "PN12QP109")
    N, level = 1 << logn, len(Q) - 1
    ct = _inputs(gpu_pkg, Q, N, batch, 310)
    gens = chain_ref.slot_sum_elements(N)
    keys_h = _host_keys(gpu_pkg, Q, P, N, len(gens), 420)
    got = {}
    for route, opt in (("default", None), ("no_epilogue", ring.Options(no_epilogue=1))):
        cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h, opt)
        out = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.RotateChain(level, _up(cQ, ct, batch), gens, keys, True, out)
        rep = (cQ.NewPoly(batch), cQ.NewPoly(batch))
        plan.RotateChain(level, _up(cQ, ct, batch), gens[:3], keys[:3], False, rep)
        one = _up(cQ, ct, batch)
        plan.RotateChain(level, one, gens[:1], keys[:1], True, one)          # one step in place: the addend is the output
        got[route] = [p.get() for p in out + rep + one]
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    acc, tmp = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    one = None
    for g, key in zip(gens, keys):
        plan.PermuteNTT(level, acc, g, key, tmp)           # RotateColumns
        for k in range(2):
            cQ.Add(acc[k], tmp[k], acc[k])                 # evaluator.Add
        if one is None:
            one = [p.get() for p in acc]
    rep = _up(cQ, ct, batch)
    for g, key in zip(gens[:3], keys[:3]):
        plan.PermuteNTT(level, rep, g, key, rep)
    got["steps"] = [p.get() for p in acc + rep] + one
    for route in ("no_epilogue", "steps"):
        for k in range(6):
            assert np.array_equal(got["default"][k], got[route][k]), (logn, route, k)


def test_no_step_one_key_twice_and_crossed_outputs(gpu_pkg, oracle):
    """n_steps = 0 copies, also into the other component's poly; one key handle for two steps; an output over the other component's
    input; outputs of a stride that differs between the components"""
    Q, P = _moduli(gpu_pkg, "PN12QP109", False)
    N, batch, level = 1 << 12, 2, len(Q) - 1
    ct = _inputs(gpu_pkg, Q, N, batch, 320)
    keys_h = _host_keys(gpu_pkg, Q, P, N, 1, 440)
    key_h = _as_plan(keys_h[0], Q, P, N)
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, batch, keys_h)
    c, out = _up(cQ, ct, batch), (cQ.NewPoly(batch), cQ.NewPoly(batch))
    plan.RotateChain(level, c, [], [], False, out)
    _same(out, ct, level, ("no step",))
    plan.RotateChain(level, c, [], [], True, (c[1], c[0]))
    _same((c[1], c[0]), ct, level, ("no step, crossed",))
    gens = chain_ref.slot_sum_elements(N)[:2]
    for accumulate in (True, False):
        want = _want(oplan, level, Q, ct, batch, gens, [key_h, key_h], accumulate)
        c = _up(cQ, ct, batch)
        plan.RotateChain(level, c, gens, [keys[0], keys[0]], accumulate, (c[1], c[0]))
        _same((c[1], c[0]), want, level, ("crossed", accumulate))
    # level 0 of polys with two limbs into one with one limb: three different strides in one call
    want = _want(oplan, 0, Q, ct, batch, gens, [key_h, key_h], True)
    c, out = _up(cQ, ct, batch), (cQ.NewPolyLvl(0, batch), cQ.NewPoly(batch))
    plan.RotateChain(0, c, gens, [keys[0], keys[0]], True, out)
    for k in range(2):
        assert np.array_equal(out[k].get().reshape(batch, -1, N)[:, 0], want[k][:, 0]), ("mixed strides", k)


def _slot_sum_error(pkg, options):
    """lr_keygen -> lr_ckks_encoder -> lr_ckks_encryptor -> the accumulating chain over 5^(2^i) -> decrypt -> decode at PN12QP109: the
    largest distance of a slot from the sum of the slots"""
    ring = pkg.ring
    N, Q, P = pkg.params.ckks_moduli("PN12QP109")
    Q, P, batch = [int(q) for q in Q], [int(p) for p in P], 2
    level, slots, scale = len(Q) - 1, N >> 1, 2.0 ** 40
    if options is None:
        cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    else:
        cQ, cP = ring.NewContextWithParams(N, Q, options=options), ring.NewContextWithParams(N, P, options=options)
    rng = np.random.default_rng(31)
    moduli = Q + P
    n = 2 * (N.bit_length() - 2) + 1
    kg = ring.KeyGenerator(cQ, cP, n)
    bits = lambda b: rng.integers(0, 256, (b, N >> 3)).astype(np.uint8)
    noise = lambda *shape: (rng.integers(0, 20, shape) | (rng.integers(0, 2, shape) << 7)).astype(np.uint8)
    uniform = lambda *lead: np.stack([rng.integers(0, q, lead + (N,), dtype=np.uint64) for q in moduli], axis=-2)
    sk = kg.GenSecretKey((bits(1), bits(1)), kg.NewKey())
    pk = kg.GenPublicKey(sk, noise(1, N), (kg.NewKey(), kg.NewKey().set(uniform(1))))
    rot = kg.GenRotationKeysPow2(sk, noise(n, kg.beta, N), uniform(n, kg.beta))
    gens = chain_ref.slot_sum_elements(N)
    assert [rot["left"][1 << i][0] for i in range(len(gens))] == gens
    keys = [rot["left"][1 << i][1] for i in range(len(gens))]
    coder, enc = ring.CkksEncoder(cQ, batch), ring.CkksEncryptor(cQ, cP, batch)
    plan = ring.CkksPlan(cQ, cP, batch, options=options)
    values = rng.uniform(-1, 1, (batch, slots)) + 1j * rng.uniform(-1, 1, (batch, slots))
    pt = coder.Encode(cQ.NewPoly(batch), values, level, scale)
    ct = enc.EncryptPk(pk, (bits(batch), bits(batch)), (noise(batch, N), noise(batch, N)), pt, (cQ.NewPoly(batch), cQ.NewPoly(batch)), level)
    plan.RotateChain(level, ct, gens, keys, True, ct)
    out = cQ.NewPoly(batch)
    plan.Decrypt(level, ct, sk, out)
    got = coder.Decode(out, slots, level, scale).reshape(batch, slots)
    return float(np.max(np.abs(got - values.sum(axis=1)[:, None])))


def test_slot_sum_end_to_end_on_device_made_keys(gpu_pkg):
    """every slot equals the sum of the 2048 slots.  The bound is twice the error of the same pipeline on the composed route (a plan and
    contexts with lr_options::no_epilogue), measured in this very run: the two routes give the same bits, so the bound only guards the
    test's own arithmetic.  Measured on one MI355X: 1.849e-06 on both routes, at scale 2^40 for 2048 values of modulus up to sqrt(2).
    That the composed pipeline computes the sum at all is checked against 1e-2: 2048 fresh encryption noises of about 2^12 per
    coefficient and eleven key switches' worth of about as much each, a factor sqrt(N) = 2^6 through the decoding, over the scale 2^40,
    is about 2^-11."""
    composed = _slot_sum_error(gpu_pkg, gpu_pkg.ring.Options(no_epilogue=1))
    fused = _slot_sum_error(gpu_pkg, None)
    print("slot sum error: composed %.3e, fused %.3e" % (composed, fused))
    assert composed < 1e-2
    assert fused <= 2 * composed


def test_refusals_leave_the_outputs_unwritten(gpu_pkg):
    """every refusal the header lists, with its code; argument checks come before shape checks; nothing is written"""
    ring, err = gpu_pkg.ring, gpu_pkg._native.LatticeRingError
    Q, P = _moduli(gpu_pkg, "PN13QP218", False)
    logn, nQ = 12, len(Q)
    N, level = 1 << logn, nQ - 1
    keys_h = _host_keys(gpu_pkg, Q, P, N, 1, 460)
    cQ, plan, keys = _device(gpu_pkg, Q, P, N, 1, keys_h)
    other, _, _ = _device(gpu_pkg, Q, P, N >> 1, 1, [])
    key = keys[0]
    mark = np.full((1, nQ, N), 7, dtype=np.uint64)
    c = (cQ.NewPoly(1).set(mark + 1), cQ.NewPoly(1).set(mark + 2))
    out = (cQ.NewPoly(1).set(mark), cQ.NewPoly(1).set(mark))
    big = [cQ.NewPoly(2) for _ in range(4)]
    narrow, short = cQ.NewPolyLvl(nQ - 2, 1), other.NewPoly(1)
    small_key = ring.Poly(cQ, nQ + len(P), 2)                 # beta = 6 here: 12 polys are needed
    thin_key = ring.Poly(cQ, nQ, 2 * nQ)                      # no limbs of P
    ARG, SHAPE = 4, 3

    def refused(code, call):
        with pytest.raises(err) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))
        assert all(np.array_equal(o.get().reshape(mark.shape), mark) for o in out)
    chain = lambda ct, gens, ks, o, lvl=level: plan.RotateChain(lvl, ct, gens, ks, True, o)
    lib, h, check = gpu_pkg._native.lib(), lambda p: p.h, gpu_pkg._native.check
    raw = lambda *a: check(lib.lr_ckks_rotate_chain(*a))
    refused(ARG, lambda: chain(c, [5, 25], [key, None], out))                                    # a null entry in keys
    refused(ARG, lambda: raw(plan.h, level, h(c[0]), h(c[1]), 1, None, None, 1, h(out[0]), h(out[1])))
    refused(ARG, lambda: raw(plan.h, level, h(c[0]), None, 0, None, None, 1, h(out[0]), h(out[1])))
    refused(ARG, lambda: raw(None, level, h(c[0]), h(c[1]), 0, None, None, 1, h(out[0]), h(out[1])))
    refused(ARG, lambda: raw(plan.h, level, h(c[0]), h(c[1]), 0, None, None, 1, h(out[0]), None))
    refused(ARG, lambda: raw(plan.h, level, h(c[0]), h(c[1]), -1, None, None, 1, h(out[0]), h(out[1])))
    refused(ARG, lambda: chain(c, [5, 4], [key, key], out))                                      # an even Galois element
    refused(ARG, lambda: chain(c, [5], [key], (out[0], out[0])))                                 # the same output poly twice
    refused(ARG, lambda: chain((big[0], big[1]), [5], [key], (out[0], out[0])))                  # two reasons: the argument check comes first
    refused(ARG, lambda: chain(c, [4], [key], out, nQ))                                          # ... also before the level
    refused(SHAPE, lambda: chain(c, [5], [key], out, nQ))                                        # level out of range
    refused(SHAPE, lambda: chain(c, [5], [key], out, -1))
    refused(SHAPE, lambda: chain((big[0], big[1]), [5], [key], (big[2], big[3])))                # a batch beyond max_batch
    refused(SHAPE, lambda: chain((c[0], narrow), [5], [key], out))                               # fewer limbs than level + 1
    refused(SHAPE, lambda: chain((short, c[1]), [5], [key], out))                                # another degree
    refused(SHAPE, lambda: chain(c, [5], [key], (out[0], big[0])))                               # another batch
    refused(SHAPE, lambda: chain(c, [5, 25], [key, small_key], out))                             # a key image that is too small
    refused(SHAPE, lambda: chain(c, [5], [thin_key], out))
    assert all(np.array_equal(c[k].get().reshape(mark.shape), mark + 1 + k) for k in range(2))
    plan.RotateChain(nQ - 2, (c[0], narrow), [5], [key], True, (out[0], narrow))                 # the same polys one level down: accepted
