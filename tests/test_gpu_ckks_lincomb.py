"""lr_ckks_lincomb (res = c0 + sum c_k ct_k on both components in one device call) against the sequence it replaces -- the oracle's
half_scalar_op with op 0, then per term op 1 and op 2, tests/ckks_lincomb_ref.elements -- bit for bit, at the smallest shapes where the
pass can go wrong: N = 4 (one pair per half), 16, 2^11 and 2^16 (the second trip of a lane over the pairs); batches 1 and 3, members that
lie apart by more than their limbs (views into larger polys), a level below the polys' limb count; 0 (with a constant), 1, 2, 16 and 17
terms (a second pass through the receiver) and at N = 16 with nine limbs also the second limb range of a launch; pre-multipliers on none,
some and all terms; on top of the receiver and from zero over a receiver full of garbage; words 0, 1, q - 1 and q; lo != hi; a term listed
twice; values that are not canonical (AddNoMod outputs, q, 2q - 1, 2^64 - 1); the limit moduli of tests/limit_moduli.py.  Every refusal
with its code and message and the receiver untouched; the public surface end to end (constants, the call, Rescale) against the
restatement; twelve seeded random cases."""
import ctypes as C

import numpy as np
import pytest

import ckks_lincomb_ref as ref
import limit_moduli as lm
from handle_fuzz_shapes import _moduli

pytestmark = pytest.mark.gpu

W = 1 << 64


def _words(rng, Q, special=None):
    """one word per limb below its modulus, or the special value (0, 1, q - 1, q)"""
    if special is not None:
        return np.array([{"0": 0, "1": 1, "q-1": q - 1, "q": q}[special] for q in Q], dtype=np.uint64)
    return np.array([int(rng.integers(0, q)) for q in Q], dtype=np.uint64)


def _values(rng, Q, N, batch, limbs, kind):
    """[batch, limbs, N]: canonical residues, lazy values below 2q, or anything a word holds"""
    x = np.empty((batch, limbs, N), dtype=np.uint64)
    for i, q in enumerate(Q[:limbs]):
        top = {"canonical": q, "lazy": 2 * q, "wild": W}[kind]
        x[:, i, :] = rng.integers(0, top, (batch, N), dtype=np.uint64)
        x[0, i, 0], x[0, i, N // 2] = q - 1, q          # around the conditional subtraction, on either half
        if kind != "canonical":
            x[0, i, 1], x[0, i, N - 1] = 2 * q - 1, (W - 1 if kind == "wild" else q)
    return x


class _Operand:
    """a poly of `batch` members with `limbs` limbs, dense or a view into a larger poly (members pad limbs further apart, offset one limb)"""

    def __init__(self, ring, ctx, data, strided):
        self.data = data
        batch, limbs, N = data.shape
        self.strided, self.shape = strided, data.shape
        if not strided:
            self.backing = ring.Poly(ctx, limbs, batch)
            self.poly = self.backing.set(data)
            return
        self.pad = 2
        self.backing = ring.Poly(ctx, limbs + self.pad, batch)
        full = np.full((batch, limbs + self.pad, N), 0xDEADBEEF, dtype=np.uint64)
        full[:, 1:1 + limbs, :] = data
        self.backing.set(full)
        self.full = full
        self.poly = ring.Poly.wrap_strided(ctx, self.backing.device_ptr + N * 8, limbs, batch, limbs + self.pad)

    def get(self):
        batch, limbs, N = self.shape
        if not self.strided:
            return self.backing.get().reshape(batch, limbs, N)
        got = self.backing.get().reshape(batch, limbs + self.pad, N)
        assert np.array_equal(got[:, 0], self.full[:, 0]) and np.array_equal(got[:, 1 + limbs:], self.full[:, 1 + limbs:])    # nothing around the view moved
        return got[:, 1:1 + limbs]


def _run(pkg, oracle, ctx, oc, Q, N, level, batch, T, rng, pre_on="some", accumulate=False, with_add=True, strided=False, kind="lazy", extra_limbs=0,
         specials=True, repeat=True, tag=""):
    ring = pkg.ring
    L1 = level + 1
    limbs = L1 + extra_limbs
    Ql = Q[:L1]
    datas = [(_values(rng, Q, N, batch, limbs, kind), _values(rng, Q, N, batch, limbs, kind)) for _ in range(T)]
    ops = [(_Operand(ring, ctx, d0, strided), _Operand(ring, ctx, d1, strided)) for d0, d1 in datas]
    if repeat and T >= 3:                                 # a term listed twice
        ops[2], datas[2] = ops[0], datas[0]
    garbage = (_values(rng, Q, N, batch, limbs, kind), _values(rng, Q, N, batch, limbs, kind))
    outs = (_Operand(ring, ctx, garbage[0], strided), _Operand(ring, ctx, garbage[1], strided))
    has_pre = np.array([{"none": 0, "all": 1, "some": int(rng.integers(0, 2))}[pre_on] for _ in range(T)], dtype=np.uint8)
    if pre_on == "some" and T >= 2:
        has_pre[0], has_pre[1] = 1, 0
    sp = ["0", "1", "q-1", "q"]
    pick = lambda k, j: _words(rng, Ql, sp[(k + j) % 4] if specials and k % 3 == 0 else None)
    pre = np.array([pick(k, 0) for k in range(T)], dtype=np.uint64).reshape(T, L1)
    lo = np.array([pick(k, 1) for k in range(T)], dtype=np.uint64).reshape(T, L1)
    hi = np.array([pick(k, 2) for k in range(T)], dtype=np.uint64).reshape(T, L1)
    add = (_words(rng, Ql), _words(rng, Ql, "q" if specials else None)) if with_add else None
    consts = ring.CkksLinCombConsts(level, 0.0, add, has_pre, pre, lo, hi)
    ctx.CkksLinComb(level, [(a.poly, b.poly) for a, b in ops], consts, add=add, accumulate=accumulate, out=(outs[0].poly, outs[1].poly))
    got = (outs[0].get(), outs[1].get())
    for b in range(batch):
        terms_b = [(d0[b], d1[b]) for d0, d1 in datas]
        start = (garbage[0][b], garbage[1][b]) if accumulate else None
        want = ref.elements(oc, level, terms_b, has_pre, pre, lo, hi, add=add, start=start)
        for u in range(2):
            assert np.array_equal(got[u][b, :L1], want[u]), (tag, N, level, batch, T, pre_on, accumulate, with_add, strided, kind, b, u)
            assert np.array_equal(got[u][b, L1:], garbage[u][b, L1:]), (tag, "limbs above the level", b, u)
    for a, b in ops:                                      # the terms are read only
        a.get(), b.get()


@pytest.fixture(scope="module")
def rings(gpu_pkg, oracle):
    made = {}

    def get(logn, Q):
        key = (logn, tuple(Q))
        if key not in made:
            made[key] = (gpu_pkg.ring.NewContextWithParams(1 << logn, list(Q)), oracle.Context(1 << logn, list(Q)))
        return made[key]
    return get


@pytest.mark.parametrize("logn", [2, 4, 11])
def test_parity_with_the_half_scalar_sequence(gpu_pkg, oracle, rings, logn):
    N = 1 << logn
    Q = lm.ewise_moduli(max(logn, 4))               # one limb per size class of the reductions next to the admission bounds, and a small prime
    ctx, oc = rings(logn, Q)
    rng = np.random.default_rng(100 + logn)
    top = len(Q) - 1
    for T in (0, 1, 2, 16, 17):
        _run(gpu_pkg, oracle, ctx, oc, Q, N, top, 1, T, rng, pre_on="some", accumulate=False, with_add=True, kind="lazy", tag="a")
        _run(gpu_pkg, oracle, ctx, oc, Q, N, 2, 3, T, rng, pre_on="all", accumulate=True, with_add=(T == 0 or T == 16), strided=True, kind="wild",
             extra_limbs=1, tag="b")
    _run(gpu_pkg, oracle, ctx, oc, Q, N, 3, 3, 2, rng, pre_on="none", accumulate=False, with_add=False, strided=True, kind="canonical", extra_limbs=2, tag="c")
    _run(gpu_pkg, oracle, ctx, oc, Q, N, 0, 1, 5, rng, pre_on="some", accumulate=True, with_add=True, kind="wild", tag="d")
    _run(gpu_pkg, oracle, ctx, oc, Q, N, top, 1, 0, rng, accumulate=False, with_add=False, tag="zeros")              # no term, no constant: zeros
    _run(gpu_pkg, oracle, ctx, oc, Q, N, top, 3, 0, rng, accumulate=True, with_add=False, strided=True, tag="as it is")   # ... or the receiver as it is


def test_parity_on_non_canonical_sums(gpu_pkg, oracle, rings):
    """terms and receiver that are outputs of AddNoMod (sums of two residues, up to 2q - 2)"""
    logn, N = 4, 16
    Q = lm.ewise_moduli(4)
    ctx, oc = rings(logn, Q)
    L = len(Q)
    rng = np.random.default_rng(7)
    mk = lambda s: gpu_pkg.sampling.uniform_poly(Q, N, 2, seed=s).reshape(2, L, N)
    polys, sums = [], []
    for k in range(6):
        a, b = mk(10 + 2 * k), mk(11 + 2 * k)
        a[0, :, :2] = b[0, :, :2] = np.array([q - 1 for q in Q], dtype=np.uint64)[:, None]
        pa, pb, ps = ctx.NewPoly(2).set(a), ctx.NewPoly(2).set(b), ctx.NewPoly(2)
        ctx.AddNoMod(pa, pb, ps)
        polys.append(ps)
        sums.append(a + b)
        assert np.array_equal(ps.get().reshape(2, L, N), sums[-1])
    has_pre = np.array([1, 0], dtype=np.uint8)
    pre, lo, hi = (np.array([_words(rng, Q), _words(rng, Q)], dtype=np.uint64) for _ in range(3))
    add = (_words(rng, Q), _words(rng, Q))
    consts = gpu_pkg.ring.CkksLinCombConsts(L - 1, 0.0, add, has_pre, pre, lo, hi)
    ctx.CkksLinComb(L - 1, [(polys[0], polys[1]), (polys[2], polys[3])], consts, add=add, accumulate=True, out=(polys[4], polys[5]))
    for b in range(2):
        want = ref.elements(oc, L - 1, [(sums[0][b], sums[1][b]), (sums[2][b], sums[3][b])], has_pre, pre, lo, hi, add=add, start=(sums[4][b], sums[5][b]))
        for u in range(2):
            assert np.array_equal(polys[4 + u].get().reshape(2, L, N)[b], want[u]), (b, u)


def test_parity_at_the_second_trip_of_a_lane(gpu_pkg, oracle, rings):
    """N = 2^16: 2^15 pairs on a grid of 64 workgroups, two trips per lane; batch 1, two limbs"""
    logn = 16
    Q = [lm.below(61, logn), lm.below(46, logn)]
    ctx, oc = rings(logn, Q)
    rng = np.random.default_rng(16)
    _run(gpu_pkg, oracle, ctx, oc, Q, 1 << logn, 1, 1, 2, rng, pre_on="some", accumulate=True, with_add=True, kind="wild", tag="2^16")
    _run(gpu_pkg, oracle, ctx, oc, Q, 1 << logn, 1, 1, 5, rng, pre_on="all", accumulate=False, with_add=True, strided=True, kind="lazy", tag="2^16 view")


def test_parity_over_two_limb_ranges(gpu_pkg, oracle, rings):
    """sixteen terms and a constant leave room for seven limbs in a launch's arguments: nine limbs are two launches per pass"""
    logn, N = 4, 16
    Q = list(gpu_pkg.params.ckks_moduli("PN15QP880")[1][:9])
    ctx, oc = rings(logn, Q)
    rng = np.random.default_rng(9)
    _run(gpu_pkg, oracle, ctx, oc, Q, N, 8, 2, 16, rng, pre_on="some", accumulate=False, with_add=True, kind="lazy", tag="two ranges")
    _run(gpu_pkg, oracle, ctx, oc, Q, N, 8, 1, 17, rng, pre_on="all", accumulate=True, with_add=True, strided=True, kind="wild", tag="two ranges, two passes")


def _raw(pkg, ctx, level, t0, t1, has_pre, pre, lo, hi, add_lo, add_hi, accumulate, o0, o1, n_terms=None):
    """lr_ckks_lincomb itself; polys may be None; returns (status, message)"""
    lib = pkg._native.lib()
    h = lambda p: None if p is None else p.h.value
    arr = lambda ps: None if ps is None else (C.c_void_p * max(len(ps), 1))(*[h(p) for p in ps])
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    n = (len(t0) if t0 is not None else len(t1)) if n_terms is None else n_terms
    rc = lib.lr_ckks_lincomb(None if ctx is None else ctx.h, level, n, arr(t0), arr(t1), ptr(has_pre), ptr(pre), ptr(lo), ptr(hi), ptr(add_lo), ptr(add_hi),
                             accumulate, None if o0 is None else o0.h, None if o1 is None else o1.h)
    return rc, lib.lr_last_error_string().decode()


def test_refusals_leave_the_receiver_alone(gpu_pkg, oracle, rings):
    ring = gpu_pkg.ring
    logn, N = 4, 16
    Q = lm.ewise_moduli(5)[:3]                      # (NTT-friendly up to N = 32)
    ctx, _ = rings(logn, Q)
    tiny = ring.NewContextWithParams(2, Q)
    other = ring.NewContextWithParams(32, Q)
    mk = lambda c, limbs, batch, seed: ring.Poly(c, limbs, batch).set(gpu_pkg.sampling.uniform_poly(Q[:limbs], c.N, batch, seed=seed))
    a0, a1, b0, b1 = (mk(ctx, 3, 2, s) for s in (1, 2, 3, 4))
    keep0, keep1 = gpu_pkg.sampling.uniform_poly(Q, N, 2, seed=5), gpu_pkg.sampling.uniform_poly(Q, N, 2, seed=6)
    o0, o1 = ring.Poly(ctx, 3, 2).set(keep0), ring.Poly(ctx, 3, 2).set(keep1)
    narrow, single, wide = mk(ctx, 2, 2, 7), mk(ctx, 3, 1, 8), mk(other, 3, 2, 9)
    inside = ring.Poly.wrap(ctx, o0.device_ptr + N * 8, 2, 1)
    s0, s1, s2, s3 = (mk(tiny, 3, 2, s) for s in (10, 11, 12, 13))
    hp = np.array([0, 1], dtype=np.uint8)
    k = np.arange(1, 7, dtype=np.uint64)
    top = 2
    who = "CKKS linear combination: "
    ARG, SHAPE, UNSUPPORTED = 4, 3, 6
    base = dict(ctx=ctx, level=top, t0=[a0, b0], t1=[a1, b1], has_pre=hp, pre=k, lo=k, hi=k, add_lo=k, add_hi=k, accumulate=0, o0=o0, o1=o1)
    cases = [
        (dict(ctx=None), ARG, "null argument"), (dict(o0=None), ARG, "null argument"), (dict(o1=None), ARG, "null argument"),
        (dict(n_terms=-1), ARG, "n_terms is negative"),
        (dict(t0=None), ARG, "null argument"), (dict(has_pre=None), ARG, "null argument"), (dict(pre=None), ARG, "null argument"),
        (dict(lo=None), ARG, "null argument"), (dict(hi=None), ARG, "null argument"),
        (dict(t0=[a0, None]), ARG, "a term is null"), (dict(t1=[None, b1]), ARG, "a term is null"),
        (dict(add_lo=None), ARG, "add_lo and add_hi come together or not at all"), (dict(add_hi=None), ARG, "add_lo and add_hi come together or not at all"),
        (dict(o1=o0), ARG, "the two components of the receiver share memory"), (dict(o1=inside), ARG, "the two components of the receiver share memory"),
        (dict(t1=[a1, o0], accumulate=1), ARG, "a term shares memory with the receiver"), (dict(t0=[inside, b0]), ARG, "a term shares memory with the receiver"),
        # an argument error before a shape error before the unsupported degree
        (dict(t0=[a0, None], level=9, o1=narrow), ARG, "a term is null"),
        (dict(ctx=tiny, t0=[s0], t1=[s1], o0=s2, o1=s2), ARG, "the two components of the receiver share memory"),
        (dict(ctx=tiny, level=3, t0=[s0], t1=[s1], o0=s2, o1=s3), SHAPE, "level out of range"),
        (dict(level=-1), SHAPE, "level out of range"), (dict(level=3), SHAPE, "level out of range"),
        (dict(t1=[a1, wide]), SHAPE, "ring degree mismatch"),
        (dict(t0=[a0, narrow]), SHAPE, "a poly has fewer limbs than level + 1"), (dict(o1=narrow), SHAPE, "a poly has fewer limbs than level + 1"),
        (dict(t0=[single, b0]), SHAPE, "every term and the receiver carry the same batch"), (dict(o0=single), SHAPE, "every term and the receiver carry the same batch"),
        (dict(ctx=tiny, t0=[s0], t1=[s1], o0=s2, o1=s3), UNSUPPORTED, "ring degree below 4"),
    ]
    tiny_keep = (s2.get().copy(), s3.get().copy())
    for change, code, message in cases:
        rc, msg = _raw(gpu_pkg, **dict(base, **change))
        assert (rc, msg) == (code, who + message), (change, rc, msg)
        ctx.Sync()
        assert np.array_equal(o0.get(), keep0) and np.array_equal(o1.get(), keep1), change
    tiny.Sync()
    assert np.array_equal(s2.get(), tiny_keep[0]) and np.array_equal(s3.get(), tiny_keep[1])
    with pytest.raises(ring.LatticeRingError) as e:      # ... and through the public surface
        ctx.CkksLinComb(top, [(a0, a1)], ring.CkksLinCombConsts(top, 0.0, None, hp[:1], k[:3], k[:3], k[:3]), out=(o0, o0))
    assert e.value.code == ARG
    rc, _ = _raw(gpu_pkg, **base)                      # the same arguments unchanged are accepted
    assert rc == 0
    assert not np.array_equal(o0.get(), keep0)


def test_end_to_end_through_the_public_surface(gpu_pkg, oracle):
    """N = 2^11, two CKKS-size limbs plus one: the constants from ckks_lincomb_constants for four terms of mixed scales and levels and a
    complex c0, CkksLinComb into fresh polys at level_after, CkksPlan.Rescale; against the restatement followed by the oracle's rescale"""
    ring = gpu_pkg.ring
    N = 1 << 11
    _, Qf, Pf = gpu_pkg.params.ckks_moduli("PN15QP880")
    Q, P = list(Qf[:3]), list(Pf[:1])
    cQ, cP = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, P)
    plan = ring.CkksPlan(cQ, cP, 1)
    oc = oracle.Context(N, Q)
    delta = 2.0 ** 40
    levels = [2, 1, 2, 2]
    scales = [delta * (1 + 2.0 ** -21), delta * 2, delta * (1 + 2.0 ** -20.5), delta * delta]
    cs = [0.6 - 0.3j, -3 + 0j, 0.125j + 0.7, 2 - 5j]
    c0 = 0.3 - 0.4j
    psi = cQ.GetNttPsi()[:, 1]
    assert [int(v) for v in psi] == [int(v) for v in oc.ntt_psi[:, 1]]
    terms = list(zip(cs, scales, levels))
    k = ring.ckks_lincomb_constants(Q, psi, delta, levels[0], scales[0], terms, c0)
    w = ref.constants(Q, [int(v) for v in psi], delta, levels[0], scales[0], terms, c0)
    assert (k.level_after, k.scale_after) == (w.level_after, w.scale_after) == (1, w.scale_after) and sum(w.has_pre) >= 2
    assert [[int(v) for v in r] for r in k.lo] == w.lo and [[int(v) for v in r] for r in k.pre] == w.pre and [int(v) for v in k.add[1]] == w.add[1]
    data = [(gpu_pkg.sampling.uniform_poly(Q[:l + 1], N, 1, seed=20 + 2 * i)[0], gpu_pkg.sampling.uniform_poly(Q[:l + 1], N, 1, seed=21 + 2 * i)[0])
            for i, l in enumerate(levels)]
    cts = [(cQ.NewPolyLvl(l).set(d0), cQ.NewPolyLvl(l).set(d1)) for (d0, d1), l in zip(data, levels)]
    res = (cQ.NewPolyLvl(k.level_after), cQ.NewPolyLvl(k.level_after))
    cQ.CkksLinComb(k.level_after, cts, k, add=k.add, out=res)
    want = ref.elements(oc, w.level_after, data, w.has_pre, w.pre, w.lo, w.hi, add=w.add)
    for u in range(2):
        assert np.array_equal(res[u].get().reshape(2, N), want[u]), u
    plan.Rescale(res)
    scale = k.scale_after / float(Q[k.level_after])                 # ctOut.DivScale, ckks/evaluator.go:954
    oc2 = oracle.Context(N, Q[:2])
    for u in range(2):
        assert np.array_equal(res[u].get().reshape(1, N), oc2.rescale_op("oc_div_round_by_last_modulus_ntt", want[u])), u
    assert res[0].limbs == 1 and scale > 0


@pytest.mark.parametrize("seed", range(12))
def test_seeded_fuzz(gpu_pkg, oracle, seed):
    rng = np.random.default_rng(7000 + seed)
    logn = int(rng.integers(2, 13))
    N = 1 << logn
    limbs = int(rng.integers(1, 7))
    Q = _moduli(gpu_pkg, rng, max(logn, 4), limbs)
    ctx, oc = gpu_pkg.ring.NewContextWithParams(N, Q), oracle.Context(N, Q)
    level = int(rng.integers(0, limbs))
    T = int(rng.integers(0, 21))
    if logn >= 11:
        T = min(T, 6)                                  # (the oracle's row passes are what a case costs)
    _run(gpu_pkg, oracle, ctx, oc, Q, N, level, int(rng.integers(1, 4)), T, rng, pre_on=["none", "some", "all"][int(rng.integers(0, 3))],
         accumulate=bool(rng.integers(0, 2)), with_add=bool(rng.integers(0, 2)), strided=bool(rng.integers(0, 2)),
         kind=["canonical", "lazy", "wild"][int(rng.integers(0, 3))], extra_limbs=limbs - 1 - level, tag="fuzz %d" % seed)
