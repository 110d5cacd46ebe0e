"""bfv.Evaluator.Mul for every operand degree on the device (lr_bfv_mul_deg): tensorAndRescale's branch for operands that are not both of degree
1 (bfv/evaluator.go:371-415) against its line-by-line restatement (tests/bfv_tensor_ref.py), bit for bit -- all 19 degree pairs with
1 <= d0 + d1 <= 5 and the 2 x 2 squaring, on PN12QP109, PN13QP218 and PN14QP438, on the gathered small-batch path and the per-operand one,
with and without the extension epilogues; the (1, 1) delegation, outputs over operands, every refusal, decryption with Python integers, and a
seeded fuzz family."""
import zlib

import numpy as np
import pytest

import bfv_tensor_ref as ref

pytestmark = pytest.mark.gpu

T = 65537
PAIRS = [(d0, d1) for d0 in range(6) for d1 in range(6) if 1 <= d0 + d1 <= 5 and (d0, d1) != (1, 1)]
SHAPES = [(d0, d1, False) for d0, d1 in PAIRS] + [(2, 2, True)]
# (set, logN, batch): batches 1 and 3 are gathered for every shape; 80 at N = 2^14 is per-operand for all but the three-poly shapes
# ((1, 0), (0, 1), the squaring), which LR_BFV_NO_GATHER sends there
CASES = [("PN12QP109", 12, 1), ("PN12QP109", 12, 3), ("PN13QP218", 11, 1), ("PN13QP218", 11, 3), ("PN14QP438", 14, 1), ("PN14QP438", 14, 3),
         ("PN14QP438", 14, 80)]
ENVS = [{}, {"LR_BFV_NO_GATHER": "1"}, {"LR_BFV_NO_EXT_EPILOGUE": "1"}, {"LR_BFV_NO_GATHER": "1", "LR_BFV_NO_EXT_EPILOGUE": "1"}]

_oplans, _wants = {}, {}


def _moduli(pkg, name):
    _, Q, _, QMul = pkg.params.bfv_moduli(name)
    return list(Q), list(QMul)


def _oplan(oracle, pkg, name, logn):
    if (name, logn) not in _oplans:
        Q, QMul = _moduli(pkg, name)
        _oplans[(name, logn)] = oracle.BfvPlan(oracle.Context(1 << logn, Q), oracle.Context(1 << logn, QMul), T)
    return _oplans[(name, logn)]


def _operand(Q, N, name, shape, side, k, b):
    """batch element b of poly k of side 0 (ct0) / 1 (ct1): the same values whatever the batch it is part of"""
    seed = zlib.crc32(repr((name, N, shape, side, k, b)).encode())
    return ref.uniform(Q, N, seed)


def _want(oracle, pkg, name, logn, shape, b):
    key = (name, logn, shape, b)
    if key not in _wants:
        d0, d1, sq = shape
        Q, _ = _moduli(pkg, name)
        N = 1 << logn
        a = [_operand(Q, N, name, shape, 0, i, b) for i in range(d0 + 1)]
        c = a if sq else [_operand(Q, N, name, shape, 1, j, b) for j in range(d1 + 1)]
        _wants[key] = ref.tensor_and_rescale(_oplan(oracle, pkg, name, logn), a, c, square=sq)
    return _wants[key]


def _setup(pkg, name, logn, shape, batch):
    d0, d1, sq = shape
    Q, QMul = _moduli(pkg, name)
    N = 1 << logn
    ring = pkg.ring
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)

    def up(side, k):
        return cQ.NewPoly(batch).set(np.stack([_operand(Q, N, name, shape, side, k, b) for b in range(batch)]))
    ct0 = [up(0, i) for i in range(d0 + 1)]
    ct1 = ct0 if sq else [up(1, j) for j in range(d1 + 1)]
    return cQ, cM, ct0, ct1


def _elem(p, b):
    """batch element b of a device poly, [limbs, N] (one element downloaded)"""
    return np.stack(p.get_limb_slices(b))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d%s" % (s[0], s[1], "sq" if s[2] else ""))
@pytest.mark.parametrize("name,logn,batch", CASES)
def test_mul_deg_matches_the_restatement(gpu_pkg, oracle, monkeypatch, name, logn, batch, shape):
    cQ, cM, ct0, ct1 = _setup(gpu_pkg, name, logn, shape, batch)
    nout = shape[0] + shape[1] + 1
    checked = sorted({0, batch - 1})
    for env in ENVS:
        monkeypatch.delenv("LR_BFV_NO_GATHER", raising=False)
        monkeypatch.delenv("LR_BFV_NO_EXT_EPILOGUE", raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        plan = gpu_pkg.ring.BfvPlan(cQ, cM, T, batch)
        out = [cQ.NewPoly(batch) for _ in range(nout)]
        plan.MulDeg(ct0, ct1, out)
        for b in checked:
            want = _want(oracle, gpu_pkg, name, logn, shape, b)
            for k in range(nout):
                assert np.array_equal(_elem(out[k], b), want[k]), (env, b, k)


@pytest.mark.parametrize("name,logn,batch", [("PN13QP218", 11, 3), ("PN14QP438", 14, 80)])
def test_squaring_equals_the_product_of_two_copies(gpu_pkg, name, logn, batch):
    shape = (2, 2, True)
    cQ, cM, ct0, _ = _setup(gpu_pkg, name, logn, shape, batch)
    plan = gpu_pkg.ring.BfvPlan(cQ, cM, T, batch)
    copies = [p.CopyNew() for p in ct0]
    sq, reg = [cQ.NewPoly(batch) for _ in range(5)], [cQ.NewPoly(batch) for _ in range(5)]
    plan.MulDeg(ct0, ct0, sq)
    plan.MulDeg(ct0, copies, reg)
    for k in range(5):
        assert np.array_equal(sq[k].get(), reg[k].get()), k


@pytest.mark.parametrize("name,logn,batch", [("PN12QP109", 12, 2), ("PN14QP438", 14, 80)])
def test_one_by_one_is_lr_bfv_mul(gpu_pkg, name, logn, batch):
    Q, QMul = _moduli(gpu_pkg, name)
    N = 1 << logn
    ring = gpu_pkg.ring
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)
    plan = ring.BfvPlan(cQ, cM, T, batch)
    ops = [cQ.NewPoly(batch).set(gpu_pkg.sampling.uniform_poly(Q, N, batch, seed=60 + k).reshape(batch, len(Q), N)) for k in range(4)]
    for a, b in ((ops[:2], ops[2:]), (ops[:2], ops[:2])):
        o1, o2 = [cQ.NewPoly(batch) for _ in range(3)], [cQ.NewPoly(batch) for _ in range(3)]
        plan.Mul(a, b, o1)
        plan.MulDeg(a, b, o2)
        for k in range(3):
            assert np.array_equal(o1[k].get(), o2[k].get()), k


def test_ciphertext_times_plaintext_over_the_ciphertext(gpu_pkg, oracle):
    """bfv_test.go:478 (CtPlain): Mul(ct, pt, ct) -- the product written over the ciphertext operand"""
    name, logn, batch = "PN12QP109", 12, 3
    shape = (1, 0, False)
    cQ, cM, ct0, ct1 = _setup(gpu_pkg, name, logn, shape, batch)
    plan = gpu_pkg.ring.BfvPlan(cQ, cM, T, batch)
    plan.MulDeg(ct0, ct1, ct0)
    for b in (0, 2):
        want = _want(oracle, gpu_pkg, name, logn, shape, b)
        for k in range(2):
            assert np.array_equal(_elem(ct0[k], b), want[k]), (b, k)


def test_refusals(gpu_pkg):
    Q, QMul = _moduli(gpu_pkg, "PN12QP109")
    N = 1 << 12
    ring, nat = gpu_pkg.ring, gpu_pkg._native
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)
    plan = ring.BfvPlan(cQ, cM, T, 2)
    def P(batch=2, limbs=None):
        p = cQ.NewPoly(batch) if limbs is None else ring.Poly(cQ, limbs, batch)
        p.Zero()
        return p
    a, b = [P() for _ in range(3)], [P() for _ in range(2)]
    o = [P() for _ in range(4)]

    def code(ct0, ct1, out):
        with pytest.raises(nat.LatticeRingError) as e:
            plan.MulDeg(ct0, ct1, out)
        return e.value.code
    assert code([a[0]], [b[0]], [o[0]]) == 4                                    # degree sum 0
    assert code(a + [b[0]], a + [b[0]], [P() for _ in range(7)]) == 4           # degree sum 6
    assert code(a, b, [o[0], o[1], o[2], o[1]]) == 4                            # duplicate outputs
    assert code(a, [b[0], None], o) == 4                                        # null
    assert code(a, b, o[:3]) == 4                                               # too few outputs (caught before the call)
    assert code([P(3), P(3)], [P(3)], [P(3), P(3)]) == 3                        # batch above max_batch
    assert code(a, [b[0], P(limbs=len(Q) - 1)], o) == 3                         # limb mismatch
    assert code(a, [b[0], P(1)], o) == 3                                        # batch mismatch
    with pytest.raises(nat.LatticeRingError) as e:                              # lr_bfv_mul: duplicate outputs
        plan.Mul(a[:2], b, [o[0], o[1], o[0]])
    assert e.value.code == 4 and "distinct" in str(e.value)
    # the plan stays usable after its refusals
    plan.MulDeg(a[:2], [b[0]], o[:2])


@pytest.mark.parametrize("kind", ["ct_x_pt", "deg2_x_deg1"])
def test_device_product_decrypts(gpu_pkg, oracle, kind):
    """Python integers decide: ct x pt on PN12QP109 decrypts to m0 m; a degree-2 result times a ciphertext on PN13QP218's moduli at
    logN 11 decrypts against (1, s, s^2, s^3) to m0 m1 m2"""
    name, logn = ("PN12QP109", 12) if kind == "ct_x_pt" else ("PN13QP218", 11)
    Q, QMul = _moduli(gpu_pkg, name)
    N = 1 << logn
    ocQ = oracle.Context(N, Q)
    ring = gpu_pkg.ring
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)
    plan = ring.BfvPlan(cQ, cM, T, 1)
    up = lambda x: cQ.NewPoly(1).set(x)
    s = ref.small(N, 1, 71)
    ms = [np.random.default_rng(72 + k).integers(0, T, size=N) for k in range(3)]
    ct = [up(x) for x in ref.encrypt(ocQ, T, s, ms[0], 300)]
    if kind == "ct_x_pt":
        out = [cQ.NewPoly(1) for _ in range(2)]
        plan.MulDeg(ct, [up(ref.encode(Q, T, ms[1]))], out)
        want = ref.negacyclic(ms[0], ms[1], T)
    else:
        ct1 = [up(x) for x in ref.encrypt(ocQ, T, s, ms[1], 310)]
        ct2 = [up(x) for x in ref.encrypt(ocQ, T, s, ms[2], 320)]
        c2 = [cQ.NewPoly(1) for _ in range(3)]
        plan.Mul(ct, ct1, c2)
        out = [cQ.NewPoly(1) for _ in range(4)]
        plan.MulDeg(c2, ct2, out)
        want = ref.negacyclic(ref.negacyclic(ms[0], ms[1], T), ms[2], T)
    assert ref.decrypt(ocQ, T, [p.get() for p in out], s) == want


def test_fuzz_shapes_batches_and_aliasing(gpu_pkg, oracle):
    """40 seeded cases: a random degree pair (or the squaring), parameter set, batch and aliasing pattern (outputs over operands)"""
    rng = np.random.default_rng(20261016)
    sets = [("PN12QP109", 12), ("PN13QP218", 11), ("PN14QP438", 14)]
    ring = gpu_pkg.ring
    for case in range(40):
        shape = SHAPES[rng.integers(len(SHAPES))]
        name, logn = sets[rng.integers(len(sets))]
        batch = int(rng.choice([1, 2, 3, 5, 9] + ([40, 90] if logn < 14 else [33])))
        d0, d1, sq = shape
        cQ, cM, ct0, ct1 = _setup(gpu_pkg, name, logn, shape, batch)
        plan = ring.BfvPlan(cQ, cM, T, batch)
        nout = d0 + d1 + 1
        operands = ct0 + ([] if sq else ct1)
        out = [cQ.NewPoly(batch) for _ in range(nout)]
        # aliasing: each output over a distinct operand poly with probability 1/2
        free = list(range(len(operands)))
        rng.shuffle(free)
        for k in range(nout):
            if free and rng.integers(2):
                out[k] = operands[free.pop()]
        plan.MulDeg(ct0, ct1, out)
        for b in sorted({0, batch - 1}):
            want = _want(oracle, gpu_pkg, name, logn, shape, b)
            for k in range(nout):
                assert np.array_equal(_elem(out[k], b), want[k]), (case, name, shape, batch, b, k)
