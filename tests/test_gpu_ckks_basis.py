"""lr_ckks_power_basis (the products of computePowerBasis / computePowerBasisCheby as one device call) against tests/ckks_basis_ref.py --
the oracle's mulrelin and DivRoundByLastModulusNTT per product and integer arithmetic for the Chebyshev tail -- and against the composed
device sequence (MulRelin, Rescale, CkksCombine per product), bit for bit: a layer of four products on PN13QP218 with four levels
consumed, the assembly transforms of N = 2^15 and 2^16, small rings and a no_epilogue plan on the composed route, a layer cut into chunks,
products at level 0 without a division, C[1] below the top level, twelve calls without a synchronisation between them, inputs left alone,
limbs above level_after left alone, and every refusal of the header in its order.  Inputs are uniform with 0 and q - 1 planted."""
import ctypes as C

import numpy as np
import pytest

import ckks_basis_ref as ref

pytestmark = pytest.mark.gpu

ARG, SHAPE = 4, 3
SENTINEL = 0x5EED

# name -> parameter set, |Q| and |P| kept (None: all), log2(N), targets
SHAPES = {
    "pn13": ("PN13QP218", None, None, 13, [2, 3, 4, 5, 6, 7, 8, 16]),
    "pn15": ("PN15QP880", 4, 1, 15, [2, 3, 4, 5, 6, 7, 8]),
    "pn16": ("PN16QP1761", 3, 1, 16, [2, 3, 4]),
    "n10": ("PN15QP880", 4, 1, 10, [2, 3, 4, 5, 6, 7, 8]),
    "n3": ("PN15QP880", 4, 1, 3, [2, 3, 4, 5, 6, 7, 8]),
    "pn12": ("PN12QP109", None, None, 12, [2, 3, 4]),
}


def _ring_of(pkg, shape):
    name, nq, np_, logn, targets = SHAPES[shape]
    _, Q, P = pkg.params.ckks_moduli(name)
    Q, P = [int(q) for q in Q][:nq], [int(p) for p in P][:np_]
    return name, Q, P, 1 << logn, targets


def _inputs(pkg, Q, N, batch, seed):
    """C[1]: uniform polys over all of Q with zeros and q - 1 planted"""
    ct = [pkg.sampling.uniform_poly(Q, N, batch, seed=seed + k).reshape(batch, len(Q), N) for k in range(2)]
    top = np.array(Q, dtype=np.uint64) - 1
    ct[0][0, :, min(3, N - 1)] = 0
    ct[1][0, :, min(5, N - 1)] = 0
    ct[0][-1, :, N - 1] = top
    ct[1][-1, :, 0] = top
    ct[0][0, :, 1] = top
    ct[1][0, :, 1] = top
    return ct


def _evk(pkg, Q, P, N):
    beta = -(-len(Q) // len(P))
    return pkg.sampling.uniform_poly(Q + P, N, 2 * beta, seed=99), beta


_wanted = {}


def _want(pkg, oracle, shape, chebyshev, batch, c1_level):
    """the helper's basis, computed once per case and shared: (its products, C[1], per batch member {n: [2][level_after + 1, N]})"""
    key = (shape, chebyshev, batch, c1_level)
    if key not in _wanted:
        name, Q, P, N, targets = _ring_of(pkg, shape)
        delta = ref.DEFAULT_SCALE[name]
        products = ref.schedule(Q, delta, chebyshev, c1_level, delta, targets)
        ct = _inputs(pkg, Q, N, batch, 500)
        evk, beta = _evk(pkg, Q, P, N)
        el = ref.Elements(oracle, N, Q, P, evk.reshape(beta, 2, len(Q) + len(P), N))
        _wanted[key] = (products, ct, [el.run(products, c1_level, [ct[0][b], ct[1][b]]) for b in range(batch)])
    return _wanted[key]


def _device(pkg, shape, max_batch, options=None):
    ring = pkg.ring
    _, Q, P, N, _ = _ring_of(pkg, shape)
    kw = {} if options is None else {"options": options}
    cQ, cP = ring.NewContextWithParams(N, Q, **kw), ring.NewContextWithParams(N, P, **kw)
    plan = ring.CkksPlan(cQ, cP, max_batch, options=options)
    evk, _ = _evk(pkg, Q, P, N)
    return cQ, plan, plan.NewSwitchingKey().set(evk)


def _outputs(pkg, cQ, sched, batch, spare):
    """outs[k] with level_after + 1 (+ spare, up to |Q|) limbs, filled with a sentinel"""
    outs = []
    for p in sched.products:
        limbs = min(p.level_after + 1 + spare, len(cQ.Modulus))
        pair = tuple(pkg.ring.Poly(cQ, limbs, batch).set(np.full((batch, limbs, cQ.N), SENTINEL + u, dtype=np.uint64)) for u in range(2))
        outs.append(pair)
    return outs


def _check_outputs(sched, outs, want, batch, where):
    for k, p in enumerate(sched.products):
        L1 = p.level_after + 1
        for u in range(2):
            got = outs[k][u].get().reshape(batch, -1, outs[k][u].N)
            for b in range(batch):
                assert np.array_equal(got[b, :L1], want[b][int(p.n)][u]), where + (int(p.n), u, b)
            assert (got[:, L1:] == SENTINEL + u).all(), where + (int(p.n), u, "limbs above level_after")


def _composed(cQ, plan, sched, c1, evk, batch):
    """the device sequence the call stands for: per product MulRelin at mul_level, Rescale n_rescales times, the CkksCombine of the tail"""
    Cn, outs = {1: c1}, []
    for k, p in enumerate(sched.products):
        t = (cQ.NewPolyLvl(p.mul_level, batch), cQ.NewPolyLvl(p.mul_level, batch))
        plan.MulRelin(p.mul_level, Cn[int(p.a)], Cn[int(p.b)], evk, t)
        for _ in range(p.n_rescales):
            plan.Rescale(t)
        L1 = p.level_after + 1
        if p.tail == 1:
            m = sched.mult[k][:L1]
            cQ.CkksCombine("SUB", p.level_after, t, c1, t, double_a=True, ma=m if p.mult_side == 1 else None, mb=m if p.mult_side == 2 else None)
        elif p.tail == 2:
            cQ.CkksCombine("SUB", p.level_after, t, None, t, double_a=True, add=(sched.add[k][:L1], sched.add[k][:L1]))
        Cn[int(p.n)] = t
        outs.append(t)
    return outs


def _run_case(pkg, oracle, shape, chebyshev, batch, max_batch=None, options=None, c1_level=None, spare=1, composed=True):
    ring = pkg.ring
    name, Q, P, N, targets = _ring_of(pkg, shape)
    delta = ref.DEFAULT_SCALE[name]
    level = len(Q) - 1 if c1_level is None else c1_level
    products, ct, want = _want(pkg, oracle, shape, chebyshev, batch, level)
    sched = ring.ckks_power_basis_schedule(Q, delta, chebyshev, level, delta, targets)
    assert [tuple(getattr(g, f) for f in ref.Product.FIELDS) for g in sched.products] == [w.fields() for w in products]
    cQ, plan, evk = _device(pkg, shape, max_batch or 4 * batch, options)
    c1 = (cQ.NewPoly(batch).set(ct[0]), cQ.NewPoly(batch).set(ct[1]))
    outs = _outputs(pkg, cQ, sched, batch, spare)
    limbs_before = [(o[0].limbs, o[1].limbs) for o in outs]
    plan.PowerBasis(level, c1, sched, evk, outs)
    where = (shape, chebyshev, batch, max_batch)
    _check_outputs(sched, outs, want, batch, where)
    assert [(o[0].limbs, o[1].limbs) for o in outs] == limbs_before, where                     # the logical limb counts are left alone
    for u in range(2):
        assert np.array_equal(c1[u].get().reshape(ct[u].shape), ct[u]), where + ("inputs", u)
    if composed:
        seq = _composed(cQ, plan, sched, c1, evk, batch)
        for k, p in enumerate(sched.products):
            for u in range(2):
                got = outs[k][u].get().reshape(batch, -1, N)[:, :p.level_after + 1]
                assert np.array_equal(got, seq[k][u].get().reshape(batch, -1, N)[:, :p.level_after + 1]), where + ("composed", int(p.n), u)
    return sched, products


@pytest.mark.parametrize("chebyshev", [1, 0])
@pytest.mark.parametrize("batch", [1, 3])
def test_pn13_a_layer_of_four_and_four_levels(gpu_pkg, oracle, chebyshev, batch):
    sched, _ = _run_case(gpu_pkg, oracle, "pn13", chebyshev, batch)
    assert sorted(p.level_after for p in sched.products) == [1, 2, 2, 2, 2, 3, 3, 4]
    assert sum(1 for p in sched.products if p.layer == 3) == 4


@pytest.mark.parametrize("shape,chebyshev,batch", [("pn15", 1, 1), ("pn15", 1, 2), ("pn16", 1, 1), ("pn16", 0, 1)])
def test_the_assembly_transforms(gpu_pkg, oracle, shape, chebyshev, batch):
    _run_case(gpu_pkg, oracle, shape, chebyshev, batch)


@pytest.mark.parametrize("shape", ["n10", "n3"])
def test_small_rings_take_the_composed_route(gpu_pkg, oracle, shape):
    _run_case(gpu_pkg, oracle, shape, 1, 2)


@pytest.mark.parametrize("factor", [2, 1])
def test_a_layer_in_chunks(gpu_pkg, oracle, factor):
    """max_batch = 2 batch: the layer of four in two chunks; max_batch = batch: one product at a time"""
    _run_case(gpu_pkg, oracle, "pn13", 1, 3, max_batch=3 * factor)


def test_a_no_epilogue_plan_takes_the_composed_route(gpu_pkg, oracle):
    _run_case(gpu_pkg, oracle, "pn13", 1, 1, options=gpu_pkg.ring.Options(no_epilogue=1))
    _run_case(gpu_pkg, oracle, "pn13", 0, 1, options=gpu_pkg.ring.Options(no_epilogue=1), spare=0)


def test_pn12_products_at_level_0(gpu_pkg, oracle):
    """C[2] comes down to level 0; C[3] and C[4] are MulRelin at level 0 and no division"""
    sched, _ = _run_case(gpu_pkg, oracle, "pn12", 0, 2, spare=0)
    assert [(int(p.n), p.mul_level, p.n_rescales) for p in sched.products] == [(2, 1, 1), (3, 0, 0), (4, 0, 0)]


@pytest.mark.parametrize("batch", [2, 8])
def test_a_basis_whose_widest_chunk_is_a_pair(gpu_pkg, oracle, batch):
    """C[3] and C[4] as one chunk of two: merged at 2 ciphertexts, product by product at 8 (the shape measured level with the sequence)"""
    _run_case(gpu_pkg, oracle, "pn12", 1, batch, max_batch=2 * batch, spare=0)


@pytest.mark.parametrize("chebyshev", [1, 0])
def test_c1_below_the_top_level(gpu_pkg, oracle, chebyshev):
    """C[1]'s polys hold all of Q, the call runs three levels down"""
    _run_case(gpu_pkg, oracle, "pn13", chebyshev, 1, c1_level=3)


def test_calls_without_a_synchronisation_between_them(gpu_pkg, oracle):
    """The tables of a merged chunk travel through eight pinned slots that an event guards: a later call must not rewrite words an
    earlier call's copy may still read.  Twelve calls on ONE merging plan (max_batch = 4 batch: the pair C[3], C[4] and the layer of
    four are one chunk each), queued without a synchronisation: 20 chunks, so the slots wrap more than twice.  The schedules differ
    (Chebyshev and monomial; the whole list and its first three targets, one chunk instead of two), so the chunks shift against the
    slots and every slot holds the small table of a pair and later the larger one of the four: slots grow, and device images are
    rewritten in stream order.  Every call has outputs of its own, all checked afterwards."""
    pkg = gpu_pkg
    ring = pkg.ring
    name, Q, P, N, targets = _ring_of(pkg, "pn13")
    delta, level, batch = ref.DEFAULT_SCALE[name], len(Q) - 1, 3
    cQ, plan, evk = _device(pkg, "pn13", 4 * batch)
    inputs = {}
    for chebyshev in (1, 0):
        _, ct, want = _want(pkg, oracle, "pn13", chebyshev, batch, level)
        inputs[chebyshev] = ((cQ.NewPoly(batch).set(ct[0]), cQ.NewPoly(batch).set(ct[1])), want)
    runs, chunks = [], 0
    for i in range(12):
        chebyshev, short = (1, 0, 1, 0, 1, 0)[i % 6], i % 3 == 2
        sched = ring.ckks_power_basis_schedule(Q, delta, chebyshev, level, delta, targets[:3] if short else targets)
        layers = {}
        for p in sched.products:
            layers[p.layer] = layers.get(p.layer, 0) + 1
        chunks += sum(1 for width in layers.values() if width > 1)
        runs.append((i, chebyshev, sched, _outputs(pkg, cQ, sched, batch, 1)))
    assert chunks == 20                                                      # more than twice the eight slots
    for i, chebyshev, sched, outs in runs:
        plan.PowerBasis(level, inputs[chebyshev][0], sched, evk, outs)
    for i, chebyshev, sched, outs in runs:
        _check_outputs(sched, outs, inputs[chebyshev][1], batch, ("back to back", i, chebyshev))


def test_an_empty_basis_is_no_error(gpu_pkg):
    """targets [] or [1] (a polynomial of degree 2): nothing to compute, the call checks its operands and returns"""
    pkg = gpu_pkg
    name, Q, P, N, _ = _ring_of(pkg, "n10")
    cQ, plan, evk = _device(pkg, "n10", 2)
    c1 = (cQ.NewPoly(2), cQ.NewPoly(2))
    for targets in ([], [1], pkg.ring.ckks_power_basis_targets(2, True)):
        sched = pkg.ring.ckks_power_basis_schedule(Q, ref.DEFAULT_SCALE[name], 1, len(Q) - 1, ref.DEFAULT_SCALE[name], targets)
        assert sched.products == [] and plan.PowerBasis(len(Q) - 1, c1, sched, evk, []) == []


def test_every_refusal_in_the_headers_order(gpu_pkg, oracle):
    pkg = gpu_pkg
    ring, lib = pkg.ring, pkg._native.lib()
    name, Q, P, N, targets = _ring_of(pkg, "n10")
    delta, top, batch = ref.DEFAULT_SCALE[name], len(Q) - 1, 2
    cQ, plan, evk = _device(pkg, "n10", batch)
    sched = ring.ckks_power_basis_schedule(Q, delta, 1, top, delta, [2, 3, 4])
    n = len(sched.products)
    c1 = (cQ.NewPoly(batch), cQ.NewPoly(batch))
    outs = _outputs(pkg, cQ, sched, batch, 1)
    mult, add = np.ascontiguousarray(sched.mult), np.ascontiguousarray(sched.add)
    who = "CKKS power basis: "

    def call(products=None, count=n, c1_=c1, key=evk, o0=None, o1=None, row_words=len(Q), level=top, plan_=plan, mult_=mult, add_=add, nulls=()):
        prods = (pkg._native.BasisProduct * max(len(sched.products), 1))(*(products or sched.products))
        h = lambda p: None if p is None else p.h.value
        a0 = (C.c_void_p * n)(*[h(o[0]) for o in outs]) if o0 is None else (C.c_void_p * len(o0))(*[h(p) for p in o0])
        a1 = (C.c_void_p * n)(*[h(o[1]) for o in outs]) if o1 is None else (C.c_void_p * len(o1))(*[h(p) for p in o1])
        arg = {"plan": plan_.h, "products": prods, "mult": mult_.ctypes.data_as(C.c_void_p), "add": add_.ctypes.data_as(C.c_void_p), "c0": c1_[0].h,
               "c1": c1_[1].h, "evk": key.h, "o0": a0, "o1": a1}
        for x in nulls:
            arg[x] = None
        rc = lib.lr_ckks_power_basis(arg["plan"], count, arg["products"], arg["mult"], arg["add"], row_words, level, arg["c0"], arg["c1"], arg["evk"],
                                     arg["o0"], arg["o1"])
        return rc, lib.lr_last_error_string().decode()

    def spoiled(k, **fields):
        v = [pkg._native.BasisProduct.from_buffer_copy(p) for p in sched.products]
        for f, x in fields.items():
            setattr(v[k], f, x)
        return v

    # LR_ERR_ARG, in the header's order
    for x in ("plan", "c0", "c1", "evk"):
        assert call(nulls=(x,)) == (ARG, who + "null argument"), x
    assert call(count=-1) == (ARG, who + "negative product count")
    assert call(count=-1, nulls=("products",)) == (ARG, who + "negative product count")
    for x in ("products", "mult", "add", "o0", "o1"):
        assert call(nulls=(x,)) == (ARG, who + "null argument"), x
    assert call(o0=[outs[0][0], None, outs[2][0]]) == (ARG, who + "an output is null")
    assert call(o1=[outs[0][1], outs[1][1], None], row_words=1) == (ARG, who + "an output is null")
    assert call(row_words=top) == (ARG, who + "row_words is below c1_level + 1")
    bad = who + "the schedule is not self-consistent"
    for v in (spoiled(1, a=9), spoiled(0, a=3), spoiled(2, layer=1), spoiled(1, mul_level=sched.products[1].mul_level + 1),
              spoiled(0, tail=3), spoiled(1, mult_side=3), spoiled(0, n_rescales=top + 1, level_after=-1), spoiled(0, n_rescales=-1, level_after=top + 1),
              spoiled(0, level_after=top), spoiled(0, n=1), spoiled(2, n=2), spoiled(0, tail=1)):
        assert call(products=v) == (ARG, bad)
    assert call(products=spoiled(0, tail=3), row_words=top) == (ARG, who + "row_words is below c1_level + 1")      # two reasons: the earlier check
    assert call(o0=[outs[0][0], outs[1][0], outs[0][0]]) == (ARG, who + "two outputs share memory")
    assert call(o1=[outs[0][1], outs[1][0], outs[2][1]]) == (ARG, who + "two outputs share memory")
    assert call(o0=[outs[0][0], outs[1][0], c1[1]]) == (ARG, who + "an output shares memory with C[1]")
    assert call(o0=[outs[0][0], outs[0][0], c1[1]]) == (ARG, who + "two outputs share memory")
    # LR_ERR_SHAPE
    big = (cQ.NewPoly(batch + 1), cQ.NewPoly(batch + 1))
    big_outs = [(cQ.NewPoly(batch + 1), cQ.NewPoly(batch + 1)) for _ in range(n)]
    rc, msg = call(c1_=big, o0=[o[0] for o in big_outs], o1=[o[1] for o in big_outs])
    assert (rc, msg) == (SHAPE, "batch exceeds the plan's max_batch")
    assert call(c1_=big, o0=[o[0] for o in big_outs], o1=[big_outs[0][1], big_outs[1][1], big_outs[0][1]])[0] == ARG      # the argument checks first
    assert call(count=0, level=-1) == (SHAPE, who + "level out of range")
    high = spoiled(0, mul_level=top + 1, n_rescales=0, level_after=top + 1)
    assert call(products=high, count=1, level=top + 1, row_words=top + 2) == (SHAPE, who + "level out of range")
    cO = ring.NewContextWithParams(N >> 1, Q)
    assert call(c1_=(cO.NewPoly(batch), c1[1])) == (SHAPE, "ring degree mismatch")
    assert call(c1_=(c1[0], cQ.NewPolyLvl(top - 1, batch))) == (SHAPE, "poly has fewer limbs than level+1")
    assert call(o1=[outs[0][1], cQ.NewPoly(batch + 1), outs[2][1]]) == (SHAPE, "batch mismatch")
    assert call(o1=[outs[0][1], outs[1][1], cQ.NewPolyLvl(sched.products[2].level_after - 1, batch)]) == (SHAPE, "poly has fewer limbs than level+1")
    wide = ring.Poly(cQ, outs[1][1].alloc_limbs + 1, batch) if outs[1][1].alloc_limbs < len(Q) else cQ.NewPolyLvl(sched.products[1].level_after, batch)
    assert call(o1=[outs[0][1], wide, outs[2][1]]) == (SHAPE, who + "the two polys of an output must share their stride")
    beta = -(-len(Q) // len(P))
    for key in (ring.Poly(cQ, len(Q) + len(P), 2 * beta - 1), ring.Poly(cQ, len(Q) + len(P) - 1, 2 * beta)):
        assert call(key=key) == (SHAPE, who + "evaluation key: need batch >= 2*beta and |Q|+|P| limbs")
    # nothing was written by any of them
    for k in range(n):
        for u in range(2):
            assert (outs[k][u].get() == SENTINEL + u).all()
    assert call()[0] == 0 and call(count=0, nulls=("products", "mult", "add", "o0", "o1"))[0] == 0
