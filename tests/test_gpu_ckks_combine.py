"""lr_ckks_combine (out = a (+|-) b over CKKS ciphertexts of any degree in one device call) against the sequence it replaces -- the oracle's
half_scalar_op with op 1 and op 0 and its element-wise ADD .. SUB_NOMOD, NEG and COPY, tests/ckks_combine_ref.elements -- bit for bit, at
the smallest shapes where the pass can go wrong: N = 4 (one pair per half), 16, 2^11 and 2^16 (the second trip of a lane over the pairs);
one to three limbs and a level below the polys' limb count; batches 1 and 3 and an operand of batch 1 that every member reads; every
degree pair with b present and absent; all four operations; every combination of the flags (double_a, a multiplier of a, of b, the
constant); lo != hi; the receiver fresh (over garbage), a, b, and a is b is the receiver; values in [q, 2q) and whatever a word holds, and
AddNoMod / SubNoMod outputs fed back in; the limit moduli of tests/limit_moduli.py.  Every refusal with its code and message and the
receiver untouched; the public surface end to end (constants, then the call) for the Chebyshev step with unequal scales and levels against
the line-by-line model; twelve seeded random cases."""
import ctypes as C
import itertools

import numpy as np
import pytest

import ckks_combine_ref as ref
import limit_moduli as lm
from handle_fuzz_shapes import _moduli

pytestmark = pytest.mark.gpu

W = 1 << 64


def _words(rng, Q):
    return np.array([int(rng.integers(0, q)) for q in Q], dtype=np.uint64)


def _values(rng, Q, N, batch, limbs, kind):
    """[batch, limbs, N]: canonical residues, lazy values below 2q, or anything a word holds"""
    x = np.empty((batch, limbs, N), dtype=np.uint64)
    for i, q in enumerate(Q[:limbs]):
        top = {"canonical": q, "lazy": 2 * q, "wild": W}[kind]
        x[:, i, :] = rng.integers(0, top, (batch, N), dtype=np.uint64)
        x[0, i, 0], x[0, i, N // 2] = q - 1, 0          # around the conditional subtraction and the negated zero, on either half
        if kind != "canonical":
            x[0, i, 1], x[0, i, N - 1] = 2 * q - 1, (W - 1 if kind == "wild" else q)
    return x


def _run(pkg, ctx, oc, Q, N, level, batch, op, deg_a, deg_b, rng, double_a=False, mult_a=False, mult_b=False, with_add=False, receiver="new",
         share=None, kind="lazy", extra_limbs=0, tag=""):
    """one call against the sequence.  deg_b = -1: no b; receiver "new" | "a" | "b" | "both" (out_u is that operand's poly where it has
    one); share "a" | "b": that operand has batch 1 and every member reads it"""
    ring = pkg.ring
    L1 = level + 1
    limbs = L1 + extra_limbs
    Ql = Q[:L1]
    comps = max(deg_a, deg_b) + 1
    batch_of = lambda side: 1 if share == side else batch
    da = [_values(rng, Q, N, batch_of("a"), limbs, kind) for _ in range(deg_a + 1)]
    db = da if receiver == "both" else [_values(rng, Q, N, batch_of("b"), limbs, kind) for _ in range(deg_b + 1)]
    pa = [ring.Poly(ctx, limbs, d.shape[0]).set(d) for d in da]
    pb = pa if receiver == "both" else [ring.Poly(ctx, limbs, d.shape[0]).set(d) for d in db]
    garbage = [_values(rng, Q, N, batch, limbs, kind) for _ in range(comps)]
    own = {"new": [], "a": pa, "b": pb, "both": pa}[receiver]
    before = [(da if receiver in ("a", "both") else db)[u] if u < len(own) else garbage[u] for u in range(comps)]
    out = [own[u] if u < len(own) else ring.Poly(ctx, limbs, batch).set(garbage[u]) for u in range(comps)]
    half = lambda on: (_words(rng, Ql), _words(rng, Ql)) if on else None
    ma, mb, add = half(mult_a), half(mult_b and deg_b >= 0), half(with_add)
    ctx.CkksCombine(op, level, pa, pb if deg_b >= 0 else None, out, double_a=double_a, ma=ma, mb=mb, add=add)
    got = [p.get().reshape(batch, limbs, N) for p in out]
    what = (tag, N, level, batch, op, deg_a, deg_b, double_a, mult_a, mult_b, with_add, receiver, share, kind)
    for m in range(batch):
        want = ref.elements(oc, op, level, [d[m % d.shape[0]] for d in da], None if deg_b < 0 else [d[m % d.shape[0]] for d in db], double_a, ma, mb, add)
        for u in range(comps):
            assert np.array_equal(got[u][m, :L1], want[u]), what + (m, u)
            assert np.array_equal(got[u][m, L1:], before[u][m, L1:]), what + ("limbs above the level", m, u)
    for polys, datas in ((pa, da), (pb, db)):              # an operand that is not the receiver is read only
        for u, (p, d) in enumerate(zip(polys, datas)):
            if not any(p is o for o in out):
                assert np.array_equal(p.get().reshape(d.shape), d), what + ("operand changed", u)


@pytest.fixture(scope="module")
def rings(gpu_pkg, oracle):
    made = {}

    def get(logn, Q):
        key = (logn, tuple(Q))
        if key not in made:
            made[key] = (gpu_pkg.ring.NewContextWithParams(1 << logn, list(Q)), oracle.Context(1 << logn, list(Q)))
        return made[key]
    return get


FLAGS = list(itertools.product((False, True), repeat=4))            # double_a, mult_a, mult_b, with_add
DEGREE_PAIRS = [(da, db) for da in range(3) for db in range(-1, 3)]


@pytest.mark.parametrize("logn", [2, 4, 11])
def test_parity_with_the_sequence(gpu_pkg, oracle, rings, logn):
    N = 1 << logn
    Q = lm.ewise_moduli(max(logn, 4))[:3] if logn == 11 else lm.ewise_moduli(max(logn, 4))
    ctx, oc = rings(logn, Q)
    rng = np.random.default_rng(300 + logn)
    top = len(Q) - 1
    # every degree pair x every operation, the flags cycling; then every flag combination on one pair per operation
    for k, ((da, db), op) in enumerate(itertools.product(DEGREE_PAIRS, ref.OPS)):
        f = FLAGS[(5 * k + 3) % 16]
        _run(gpu_pkg, ctx, oc, Q, N, min(k % 3, top), 1 + 2 * (k % 2), op, da, db, rng, *f, kind=("lazy", "wild", "canonical")[k % 3],
             extra_limbs=(k % 2 if min(k % 3, top) < top else 0), tag="degrees")
    for k, (f, op) in enumerate(itertools.product(FLAGS, ref.OPS)):
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1 + k % 2, 1, rng, *f, kind="wild", tag="flags")
        _run(gpu_pkg, ctx, oc, Q, N, min(1, top), 1, op, 1, -1, rng, *f, tag="flags, no b")
    # in place: out is a, out is b, a is b is out; an operand of batch 1 read by every member
    for k, op in enumerate(ref.OPS):
        f = FLAGS[(3 * k + 7) % 16]
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, 1, rng, *f, receiver="a", tag="in place")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 2, 1, rng, *f, receiver="a", kind="wild", tag="in place")
        _run(gpu_pkg, ctx, oc, Q, N, top, 1, op, 1, 2, rng, *f, receiver="a", tag="in place, one component fresh")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, 2, rng, *f, receiver="b", tag="in place")
        _run(gpu_pkg, ctx, oc, Q, N, top, 1, op, 0, 1, rng, *f, receiver="b", kind="wild", tag="in place")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, 1, rng, *f, receiver="both", tag="a is b is out")
        _run(gpu_pkg, ctx, oc, Q, N, top, 1, op, 2, 2, rng, True, False, False, k % 2 == 0, receiver="both", kind="wild", tag="a is b is out")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, 1, rng, *f, share="b", tag="shared b")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 2, 1, rng, *f, share="a", kind="wild", tag="shared a")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, 1, rng, *f, share="a", receiver="b", tag="shared a, out is b")
        _run(gpu_pkg, ctx, oc, Q, N, top, 3, op, 1, -1, rng, *f, share="a", tag="shared a, no b")


def test_parity_on_nomod_outputs_fed_back_in(gpu_pkg, oracle, rings):
    """the unreduced sums and differences of one call are the operands of the next, in place"""
    logn, N = 4, 16
    Q = lm.ewise_moduli(4)
    ctx, oc = rings(logn, Q)
    L, top = len(Q), len(Q) - 1
    rng = np.random.default_rng(8)
    d = [_values(rng, Q, N, 2, L, "lazy") for _ in range(4)]
    a, b = [ctx.NewPoly(2).set(d[0]), ctx.NewPoly(2).set(d[1])], [ctx.NewPoly(2).set(d[2]), ctx.NewPoly(2).set(d[3])]
    ma = (_words(rng, Q), _words(rng, Q))
    want_a, want_b = [[x[m] for x in d[:2]] for m in range(2)], [[x[m] for x in d[2:]] for m in range(2)]
    for step, op in enumerate(("ADD_NOMOD", "SUB_NOMOD", "ADD_NOMOD", "SUB", "SUB_NOMOD", "ADD")):
        mult = ma if step % 2 else None
        ctx.CkksCombine(op, top, a, b, a, double_a=(step == 2), ma=mult)
        for m in range(2):
            want_a[m] = ref.elements(oc, op, top, want_a[m], want_b[m], step == 2, mult)
            for u in range(2):
                assert np.array_equal(a[u].get().reshape(2, L, N)[m], want_a[m][u]), (step, op, m, u)
        if step == 0:
            assert all(int(want_a[0][0][i][1]) == 4 * q - 2 for i, q in enumerate(Q))      # the values did leave [0, 2q)


def test_parity_at_the_second_trip_of_a_lane(gpu_pkg, oracle, rings):
    """N = 2^16: 2^15 pairs on a grid of 64 workgroups, two trips per lane; batch 1, two limbs"""
    logn = 16
    Q = [lm.below(61, logn), lm.below(46, logn)]
    ctx, oc = rings(logn, Q)
    rng = np.random.default_rng(16)
    _run(gpu_pkg, ctx, oc, Q, 1 << logn, 1, 1, "SUB", 1, 2, rng, True, True, True, True, kind="wild", tag="2^16")
    _run(gpu_pkg, ctx, oc, Q, 1 << logn, 1, 1, "ADD_NOMOD", 1, 1, rng, False, False, True, False, receiver="a", tag="2^16 in place")


def _raw(pkg, ctx, op, level, a, b, out, a_degree=None, b_degree=None, double_a=0, ma=(None, None), mb=(None, None), add=(None, None)):
    """lr_ckks_combine itself; polys and lists may be None; returns (status, message)"""
    lib = pkg._native.lib()
    arr = lambda ps: None if ps is None else (C.c_void_p * max(len(ps), 1))(*[None if p is None else p.h.value for p in ps])
    ptr = lambda w: None if w is None else w.ctypes.data_as(C.c_void_p)
    da = (len(a) - 1 if a is not None else 1) if a_degree is None else a_degree
    db = (len(b) - 1 if b is not None else 1) if b_degree is None else b_degree
    rc = lib.lr_ckks_combine(None if ctx is None else ctx.h, op, level, da, arr(a), db, arr(b), double_a, ptr(ma[0]), ptr(ma[1]), ptr(mb[0]), ptr(mb[1]),
                             ptr(add[0]), ptr(add[1]), arr(out))
    return rc, lib.lr_last_error_string().decode()


def test_refusals_leave_the_receiver_alone(gpu_pkg, oracle, rings):
    ring = gpu_pkg.ring
    logn, N = 4, 16
    Q = lm.ewise_moduli(5)[:3]                      # (NTT-friendly up to N = 32)
    ctx, _ = rings(logn, Q)
    tiny = ring.NewContextWithParams(2, Q)
    other = ring.NewContextWithParams(32, Q)
    mk = lambda c, limbs, batch, seed: ring.Poly(c, limbs, batch).set(gpu_pkg.sampling.uniform_poly(Q[:limbs], c.N, batch, seed=seed))
    a0, a1, a2, b0, b1 = (mk(ctx, 3, 2, s) for s in (1, 2, 3, 4, 5))
    keep = [gpu_pkg.sampling.uniform_poly(Q, N, 2, seed=s) for s in (6, 7, 8)]
    o0, o1, o2 = (ring.Poly(ctx, 3, 2).set(k) for k in keep)
    narrow, single, triple, wide = mk(ctx, 2, 2, 9), mk(ctx, 3, 1, 10), mk(ctx, 3, 3, 11), mk(other, 3, 2, 12)
    inside = ring.Poly.wrap(ctx, o0.device_ptr + N * 8, 2, 1)                 # from limb 1 of member 0 of o0 on: a partial overlap
    alias = ring.Poly.wrap(ctx, o0.device_ptr, 3, 1)                          # o0's first member only: the same start, another shape
    s0, s1, s2, s3 = (mk(tiny, 3, 2, s) for s in (13, 14, 15, 16))
    k = np.arange(1, 4, dtype=np.uint64)
    top = 2
    who = "CKKS combine: "
    ARG, SHAPE, UNSUPPORTED = 4, 3, 6
    base = dict(ctx=ctx, op=0, level=top, a=[a0, a1], b=[b0, b1], out=[o0, o1], ma=(k, k), mb=(k, k), add=(k, k))
    pairs = "the two words of a multiplier or of the constant come together or not at all"
    shared = "an operand shares memory with the receiver other than component by component in place"
    cases = [
        (dict(ctx=None), ARG, "null argument"), (dict(out=None), ARG, "null argument"),
        (dict(a=None), ARG, "no operand given"),
        (dict(op=4), ARG, "the operation is not LR_ADD, LR_ADD_NOMOD, LR_SUB or LR_SUB_NOMOD"), (dict(op=-1), ARG, "the operation is not LR_ADD, LR_ADD_NOMOD, LR_SUB or LR_SUB_NOMOD"),
        (dict(a_degree=3), ARG, "a degree is outside 0..2"), (dict(a_degree=-1), ARG, "a degree is outside 0..2"), (dict(b_degree=3), ARG, "a degree is outside 0..2"),
        (dict(a=[a0, None]), ARG, "a component is null"), (dict(b=[None, b1]), ARG, "a component is null"), (dict(out=[o0, None]), ARG, "a component is null"),
        (dict(b=[b0, b1, None], out=[o0, o1, o2]), ARG, "a component is null"),
        (dict(ma=(k, None)), ARG, pairs), (dict(mb=(None, k)), ARG, pairs), (dict(add=(k, None)), ARG, pairs),
        (dict(b=None), ARG, "a multiplier of b without b"),
        (dict(out=[o0, o0]), ARG, "the components of the receiver share memory"), (dict(out=[o0, inside]), ARG, "the components of the receiver share memory"),
        (dict(a=[a0, a1, a2], out=[o0, o1, alias]), ARG, "the components of the receiver share memory"),
        (dict(a=[a0, o0]), ARG, shared), (dict(b=[o1, b1]), ARG, shared), (dict(a=[inside, a1]), ARG, shared), (dict(b=[alias, b1]), ARG, shared),
        (dict(a=[o1, o0]), ARG, shared),                                         # the receiver's polys as a, crosswise
        # an argument error before a shape error before the unsupported degree
        (dict(a=[a0, None], level=9, out=[o0, narrow]), ARG, "a component is null"),
        (dict(ctx=tiny, a=[s0, s1], b=None, mb=(None, None), out=[s2, s2]), ARG, "the components of the receiver share memory"),
        (dict(ctx=tiny, level=3, a=[s0, s1], b=None, mb=(None, None), out=[s2, s3]), SHAPE, "level out of range"),
        (dict(level=-1), SHAPE, "level out of range"), (dict(level=3), SHAPE, "level out of range"),
        (dict(b=[b0, wide]), SHAPE, "ring degree mismatch"),
        (dict(a=[a0, narrow]), SHAPE, "a poly has fewer limbs than level + 1"), (dict(out=[o0, narrow]), SHAPE, "a poly has fewer limbs than level + 1"),
        (dict(out=[o0, single]), SHAPE, "the receiver's components carry one batch, an operand that batch or 1"),
        (dict(a=[a0, triple]), SHAPE, "the receiver's components carry one batch, an operand that batch or 1"),
        (dict(ctx=tiny, a=[s0, s1], b=None, mb=(None, None), out=[s2, s3]), UNSUPPORTED, "ring degree below 4"),
    ]
    tiny_keep = (s2.get().copy(), s3.get().copy())
    for change, code, message in cases:
        rc, msg = _raw(gpu_pkg, **dict(base, **change))
        assert (rc, msg) == (code, who + message), (change, rc, msg)
        ctx.Sync()
        assert all(np.array_equal(o.get(), kept) for o, kept in zip((o0, o1, o2), keep)), change
    tiny.Sync()
    assert np.array_equal(s2.get(), tiny_keep[0]) and np.array_equal(s3.get(), tiny_keep[1])
    with pytest.raises(ring.LatticeRingError) as e:      # ... and through the public surface
        ctx.CkksCombine("ADD", top, [a0, a1], [b0, b1], [o0, o0])
    assert e.value.code == ARG
    rc, _ = _raw(gpu_pkg, **dict(base, a=[a0, single]))  # an operand of batch 1 is accepted, as are the same arguments unchanged
    assert rc == 0
    assert not np.array_equal(o0.get(), keep[0]) and np.array_equal(o2.get(), keep[2])


@pytest.mark.parametrize("cn_scale_is", ["smaller", "larger", "equal"])
def test_chebyshev_step_end_to_end_through_the_public_surface(gpu_pkg, oracle, cn_scale_is):
    """N = 2^11: C[n] = 2 C[n] - C[c] of computePowerBasisCheby with unequal scales and levels.  The constants come from
    ckks_combine_constants for Sub(C[n], C[c], C[n]) (the receiver is operand a), the call is CkksCombine with double_a; against the
    line-by-line model running Add(C[n], C[n], C[n]) and Sub(C[n], C[c], C[n]) on the oracle.  And the c == 0 branch, 2 C[n] - 1, with
    AddConst's words from ckks_lincomb_constants."""
    ring = gpu_pkg.ring
    N = 1 << 11
    Q = list(gpu_pkg.params.ckks_moduli("PN15QP880")[1][:4])
    ctx, oc = ring.NewContextWithParams(N, Q), oracle.Context(N, Q)
    delta = 2.0 ** 40
    ln, lc = 2, 3                                       # C[n] one level below C[c]
    sn = {"smaller": delta * (1 + 2.0 ** -20), "larger": delta * 2.0 ** 21 * 1.75, "equal": delta * 2.0 ** 20}[cn_scale_is]
    sc = delta * 2.0 ** 20
    dn = [gpu_pkg.sampling.uniform_poly(Q[:ln + 1], N, 1, seed=40 + u)[0] for u in range(2)]
    dc = [gpu_pkg.sampling.uniform_poly(Q[:lc + 1], N, 1, seed=50 + u)[0] for u in range(2)]
    # the model
    ev = ref.Evaluator(Q, oc, delta, psi1=[int(v) for v in oc.ntt_psi[:, 1]])
    cn, cc = ref.Element(1, ln, sn, N, dn), ref.Element(1, lc, sc, N, dc)
    assert ev.chebyshev_step(cn, cc) is None
    # the library
    k = ring.ckks_combine_constants(Q, "SUB", (1, ln, sn), (1, lc, sc), (1, ln, sn), "a")
    assert (k.level_after, k.scale_after, k.degree_after) == (cn.level(), cn.scale, cn.degree()) == (ln, max(sn, sc), 1)
    assert k.mult_side == {"smaller": 1, "larger": 2, "equal": 0}[cn_scale_is]
    if k.mult_side:
        assert [int(v) for v in k.mult] == [ref.ratio_word({"smaller": 2 ** 20 - 1, "larger": 3}[cn_scale_is], q) for q in Q[:ln + 1]]
    pn, pc = [ctx.NewPolyLvl(ln).set(d) for d in dn], [ctx.NewPolyLvl(lc).set(d) for d in dc]
    ctx.CkksCombine("SUB", k.level_after, pn, pc, pn, double_a=True, ma=k.mult if k.mult_side == 1 else None, mb=k.mult if k.mult_side == 2 else None)
    for u in range(2):
        assert np.array_equal(pn[u].get().reshape(ln + 1, N), cn.array(u, ln)), u
        assert np.array_equal(pc[u].get().reshape(lc + 1, N), dc[u]), u
    # c == 0: 2 C[n] - 1 on the result, in place, no b
    add_want = ev.chebyshev_step(cn, None)
    kc = ring.ckks_lincomb_constants(Q, oc.ntt_psi[:, 1], delta, ln, k.scale_after, [], c0=-1)
    assert ([int(v) for v in kc.add[0]], [int(v) for v in kc.add[1]]) == add_want
    ctx.CkksCombine("ADD", ln, pn, None, pn, double_a=True, add=kc.add)
    for u in range(2):
        assert np.array_equal(pn[u].get().reshape(ln + 1, N), cn.array(u, ln)), u


def test_affine_head_end_to_end(gpu_pkg, oracle):
    """the head of EvaluateChebyFast / Eco, MultByConst(C[1], 2 / (b - a), C[1]) then AddConst(C[1], (-a - b) / (b - a), C[1]), as one call
    with the caller's words, here for a complex multiplier (its halves differ); against the model's two calls"""
    ring = gpu_pkg.ring
    N = 1 << 11
    Q = list(gpu_pkg.params.ckks_moduli("PN15QP880")[1][:3])
    ctx, oc = ring.NewContextWithParams(N, Q), oracle.Context(N, Q)
    delta, scale = 2.0 ** 40, 2.0 ** 40 * 1.25
    psi = [int(v) for v in oc.ntt_psi[:, 1]]
    data = [gpu_pkg.sampling.uniform_poly(Q, N, 1, seed=60 + u)[0] for u in range(2)]
    for m, c in ((2 / (8.0 - -3.0), (3.0 - 8.0) / (8.0 - -3.0)), (0.25 - 0.5j, 0.125j - 3)):
        ev = ref.Evaluator(Q, oc, delta, psi1=psi)
        c1 = ref.Element(1, 2, scale, N, data)
        add = ev.affine_head(c1, m, c)
        _, _, _, lo, hi = ev.mults[0]
        assert (lo != hi) == isinstance(m, complex)
        p = [ctx.NewPoly().set(d) for d in data]
        ctx.CkksCombine("ADD", 2, p, None, p, ma=(np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64)),
                        add=(np.array(add[0], dtype=np.uint64), np.array(add[1], dtype=np.uint64)))
        for u in range(2):
            assert np.array_equal(p[u].get().reshape(3, N), c1.array(u, 2)), (m, u)


@pytest.mark.parametrize("seed", range(12))
def test_seeded_fuzz(gpu_pkg, oracle, seed):
    rng = np.random.default_rng(9000 + seed)
    logn = int(rng.integers(2, 13))
    N = 1 << logn
    limbs = int(rng.integers(1, 7))
    Q = _moduli(gpu_pkg, rng, max(logn, 4), limbs)
    ctx, oc = gpu_pkg.ring.NewContextWithParams(N, Q), oracle.Context(N, Q)
    for case in range(4):
        level = int(rng.integers(0, limbs))
        deg_a, deg_b = int(rng.integers(0, 3)), int(rng.integers(-1, 3))
        receiver = ["new", "new", "a", "b", "both"][int(rng.integers(0, 5))]
        if deg_b < 0 and receiver in ("b", "both"):
            receiver = "a"
        if receiver == "both":
            deg_b = deg_a
        batch = int(rng.integers(1, 4))
        share = [None, None, "a", "b"][int(rng.integers(0, 4))]
        if batch == 1 or share == receiver or receiver == "both" or (share == "b" and deg_b < 0):
            share = None
        _run(gpu_pkg, ctx, oc, Q, N, level, batch, ref.OPS[int(rng.integers(0, 4))], deg_a, deg_b, rng, *[bool(rng.integers(0, 2)) for _ in range(4)],
             receiver=receiver, share=share, kind=["canonical", "lazy", "wild"][int(rng.integers(0, 3))], extra_limbs=limbs - 1 - level,
             tag="fuzz %d.%d" % (seed, case))
