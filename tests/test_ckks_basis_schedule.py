"""lr_ckks_power_basis_schedule (the scalar side of computePowerBasis / computePowerBasisCheby, host only: no device is needed) against the
restatement in tests/ckks_basis_ref.py, every field and every word: the five CKKS parameter sets at their default scales, the Fast and
Eco target lists of degrees 5 .. 65 and their monomial twins, C[1] with the scale the affine head leaves, below the top level, with a
scale that makes a product rescale twice, the level-0 stall of PN12QP109, duplicate targets and a target of 1, the capacity protocol and
every refusal in the header's order with nothing written; and the property the merged route of lr_ckks_power_basis rests on.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import ckks_basis_ref as ref

ARG = 4
SETS = ["PN12QP109", "PN13QP218", "PN14QP438", "PN15QP880", "PN16QP1761"]
WHO = "CKKS power basis schedule: "


def _moduli(pkg, name):
    return [int(q) for q in pkg.params.ckks_moduli(name)[1]]


def _compare(pkg, moduli, delta, chebyshev, c1_level, c1_scale, targets):
    """the library against the restatement: the same products, field for field and word for word, or the refusal of the domain"""
    ring = pkg.ring
    try:
        want = ref.schedule(moduli, delta, chebyshev, c1_level, c1_scale, targets)
    except ref.DomainError as d:
        with pytest.raises(ring.LatticeRingError) as e:
            ring.ckks_power_basis_schedule(moduli, delta, chebyshev, c1_level, c1_scale, targets)
        assert e.value.code == ARG and str(e.value) == "LR_ERR_ARG: " + WHO + str(d), (targets, str(d), str(e.value))
        return None
    got = ring.ckks_power_basis_schedule(moduli, delta, chebyshev, c1_level, c1_scale, targets)
    assert len(got.products) == len(want), targets
    for g, w in zip(got.products, want):
        assert tuple(getattr(g, f) for f in ref.Product.FIELDS) == w.fields(), (chebyshev, c1_level, c1_scale, targets)
    assert got.mult.shape == got.add.shape == (len(want), len(moduli))
    assert [[int(x) for x in row] for row in got.mult] == [w.mult for w in want], targets
    assert [[int(x) for x in row] for row in got.add] == [w.add for w in want], targets
    return want


@pytest.mark.parametrize("name", SETS)
def test_default_sets_fast_and_eco_lists(pkg, name):
    moduli, delta = _moduli(pkg, name), ref.DEFAULT_SCALE[name]
    top = len(moduli) - 1
    accepted = refused = 0
    for degree in range(5, 66):
        for fast in (True, False):
            targets = ref.targets(degree, fast)
            assert pkg.ring.ckks_power_basis_targets(degree, fast) == targets
            for chebyshev in (0, 1):
                want = _compare(pkg, moduli, delta, chebyshev, top, delta, targets)
                if want is None:
                    refused += 1
                    continue
                accepted += 1
                # what the lines say, once more without the model
                assert [p.n for p in want] == sorted({t for t in targets}), targets       # these lists never recurse out of order
                for p in want:
                    assert (p.a, p.b) == (-(-p.n // 2), p.n // 2) and p.level_after == p.mul_level - p.n_rescales
                    assert p.tail == (0 if not chebyshev else 2 if p.n % 2 == 0 else 1)
                    assert p.c == (p.n % 2 if chebyshev else 0)
    assert accepted > 200
    assert (refused > 0) == (name == "PN12QP109")        # only the two-limb set stalls at level 0 and leaves the domain


def test_target_lists_are_the_reference_loops(pkg):
    t = pkg.ring.ckks_power_basis_targets
    assert t(9, True) == [2, 3, 4, 8] and t(9, False) == [2, 4, 8]
    assert t(33, True) == [2, 3, 4, 5, 6, 7, 8, 16, 32] and t(33, False) == [2, 4, 8, 16, 32]
    assert t(129, True) == list(range(2, 17)) + [32, 64, 128]
    assert t(5, True) == [2, 4] and t(5, False) == [2, 4]                            # M = 3, L = 1 either way
    assert t(2, True) == [] and t(3, True) == [2]


@pytest.mark.parametrize("name", ["PN13QP218", "PN15QP880"])
@pytest.mark.parametrize("chebyshev", [0, 1])
def test_c1_as_the_affine_head_leaves_it_and_below_the_top(pkg, name, chebyshev):
    """EvaluateCheby*'s head is MultByConst by a fraction (scale * default scale), AddConst and Rescale: C[1] one level down with the scale
    delta^2 / float64(q_top), no power of two; and C[1] further down"""
    moduli, delta = _moduli(pkg, name), ref.DEFAULT_SCALE[name]
    top = len(moduli) - 1
    head = (delta * delta) / float(moduli[top])
    assert head != 2.0 ** round(np.log2(head))
    targets = ref.targets(17, True)
    want = _compare(pkg, moduli, delta, chebyshev, top - 1, head, targets)
    assert want is not None and want[0].mul_level == top - 1
    if chebyshev:
        assert {p.mult_side for p in want if p.tail == 1} != {0}      # the scales differ: one side of the Sub is multiplied
    for level in (top - 2, 2, 1):
        _compare(pkg, moduli, delta, chebyshev, level, head, targets)
        _compare(pkg, moduli, delta, chebyshev, level, delta, targets[:3])


@pytest.mark.parametrize("chebyshev", [0, 1])
def test_a_product_that_rescales_twice(pkg, chebyshev):
    moduli, delta = _moduli(pkg, "PN15QP880"), ref.DEFAULT_SCALE["PN15QP880"]
    top = len(moduli) - 1
    want = _compare(pkg, moduli, delta, chebyshev, top, delta * 2.0 ** 20, [2, 3, 4])
    assert want[0].n_rescales == 2 and want[0].level_after == top - 2
    assert want[0].scale_after == ((delta * 2.0 ** 20) ** 2 / float(moduli[top])) / float(moduli[top - 1])


def test_the_level_0_stall(pkg):
    """PN12QP109 has two limbs: C[2] comes down to level 0, every later product multiplies there and is not divided.  The monomial basis
    is accepted with n_rescales == 0 and squared scales; the Chebyshev Sub against C[1] leaves the domain of uint64(ratio)"""
    moduli, delta = _moduli(pkg, "PN12QP109"), ref.DEFAULT_SCALE["PN12QP109"]
    want = _compare(pkg, moduli, delta, 0, 1, delta, list(range(2, 9)))
    assert [(p.n, p.mul_level, p.n_rescales) for p in want] == [(2, 1, 1)] + [(n, 0, 0) for n in range(3, 9)]
    assert want[-1].scale_after == want[2].scale_after * want[2].scale_after         # C[8] = C[4] C[4]
    assert _compare(pkg, moduli, delta, 1, 1, delta, [2]) is not None
    assert _compare(pkg, moduli, delta, 1, 1, delta, [2, 3, 4]) is not None          # ratio 2^32: still inside
    with pytest.raises(pkg.ring.LatticeRingError) as e:
        pkg.ring.ckks_power_basis_schedule(moduli, delta, 1, 1, delta, list(range(2, 9)))
    assert e.value.code == ARG and str(e.value).endswith("a scale ratio is not below 2^63")
    assert _compare(pkg, moduli, delta, 1, 1, delta, list(range(2, 9))) is None


def test_duplicate_targets_a_target_of_1_and_the_order_of_creation(pkg):
    moduli, delta = _moduli(pkg, "PN14QP438"), ref.DEFAULT_SCALE["PN14QP438"]
    top = len(moduli) - 1
    for chebyshev in (0, 1):
        want = _compare(pkg, moduli, delta, chebyshev, top, delta, [1, 7, 7, 1, 4, 13, 2])
        # 7 -> a = 4 (-> 2), b = 3; 13 -> a = 7, b = 6 (-> 3, 3)
        assert [p.n for p in want] == [2, 4, 3, 7, 6, 13]
        assert _compare(pkg, moduli, delta, chebyshev, top, delta, [1, 1]) == []
        assert _compare(pkg, moduli, delta, chebyshev, top, delta, []) == []
        # the largest target, sixteen levels of recursion
        deep = _compare(pkg, moduli, delta, 0, top, 1.0, [65535])
        assert deep[-1].n == 65535 and deep[-1].layer == 16


def test_targets_outside_32_bits_are_refused_not_wrapped(pkg):
    """the binding narrows the targets to uint32_t: 2^32 + 2 and -1 must not reach the library as 2 and 2^32 - 1"""
    moduli, delta = _moduli(pkg, "PN14QP438"), ref.DEFAULT_SCALE["PN14QP438"]
    for bad in ((1 << 32) + 2, -1, 0, 65536, 1 << 40):
        with pytest.raises(pkg.ring.LatticeRingError) as e:
            pkg.ring.ckks_power_basis_schedule(moduli, delta, 0, len(moduli) - 1, delta, [2, bad])
        assert e.value.code == ARG and str(e.value) == "LR_ERR_ARG: " + WHO + "a target is 0 or above 65535", bad


def _raw(pkg, moduli, delta, chebyshev, c1_level, c1_scale, targets, capacity, n_moduli=None, nulls=()):
    """lr_ckks_power_basis_schedule itself with sentinels in every output; returns (status, message, *n_products, outputs untouched?)"""
    lib = pkg._native.lib()
    nm = len(moduli) if n_moduli is None else n_moduli
    m = (C.c_uint64 * max(len(moduli), 1))(*moduli)
    t = (C.c_uint32 * max(len(targets), 1))(*targets)
    rows = max(capacity, 1)
    count = C.c_int(-7)
    prods = (pkg._native.BasisProduct * rows)()
    C.memset(prods, 0xA5, C.sizeof(prods))
    mult, add = np.full((rows, max(nm, 1)), 0xA5A5, dtype=np.uint64), np.full((rows, max(nm, 1)), 0x5A5A, dtype=np.uint64)
    arg = {"moduli": m, "targets": t, "n_products": C.byref(count), "products": prods, "mult": mult.ctypes.data_as(C.c_void_p),
           "add": add.ctypes.data_as(C.c_void_p)}
    for n in nulls:
        arg[n] = None
    rc = lib.lr_ckks_power_basis_schedule(arg["moduli"], nm, float(delta), chebyshev, c1_level, float(c1_scale), len(targets), arg["targets"],
                                          capacity, arg["n_products"], arg["products"], arg["mult"], arg["add"])
    untouched = bytes(prods) == b"\xa5" * C.sizeof(prods) and bool((mult == 0xA5A5).all() and (add == 0x5A5A).all())
    return rc, lib.lr_last_error_string().decode(), count.value, untouched


def test_the_capacity_protocol(pkg):
    moduli, delta = _moduli(pkg, "PN15QP880"), ref.DEFAULT_SCALE["PN15QP880"]
    top = len(moduli) - 1
    targets = ref.targets(33, True)
    for capacity, nulls in ((0, ("products", "mult", "add")), (0, ()), (8, ())):
        rc, msg, count, untouched = _raw(pkg, moduli, delta, 1, top, delta, targets, capacity, nulls=nulls)
        assert (rc, msg, count, untouched) == (ARG, WHO + "more products than capacity", 9, True), (capacity, nulls)
    rc, _, count, untouched = _raw(pkg, moduli, delta, 1, top, delta, targets, 9)
    assert (rc, count, untouched) == (0, 9, False)
    # a larger buffer: the rows beyond the products stay as they were
    lib = pkg._native.lib()
    m, t, n = (C.c_uint64 * len(moduli))(*moduli), (C.c_uint32 * len(targets))(*targets), C.c_int(0)
    prods = (pkg._native.BasisProduct * 11)()
    mult, add = np.full((11, len(moduli)), 7, dtype=np.uint64), np.full((11, len(moduli)), 7, dtype=np.uint64)
    assert lib.lr_ckks_power_basis_schedule(m, len(moduli), delta, 1, top, delta, len(targets), t, 11, C.byref(n), prods,
                                            mult.ctypes.data_as(C.c_void_p), add.ctypes.data_as(C.c_void_p)) == 0
    assert n.value == 9 and (mult[9:] == 7).all() and (add[9:] == 7).all()
    # rows that are not used are zero: tail 2 has no multiplier, tail 1 no addend, and no word lies above level_after
    for k in range(9):
        p = prods[k]
        assert (mult[k, p.level_after + 1:] == 0).all() and (add[k, p.level_after + 1:] == 0).all()
        assert (add[k] == 0).all() if p.tail == 1 else (mult[k] == 0).all()
        assert p.tail != 2 or (add[k, :p.level_after + 1] != 0).all()
    # an empty basis is no refusal
    assert _raw(pkg, moduli, delta, 1, top, delta, [1], 0, nulls=("products", "mult", "add"))[::2] == (0, 0)


def test_every_refusal_in_the_headers_order_writes_nothing(pkg):
    moduli, delta = _moduli(pkg, "PN15QP880"), ref.DEFAULT_SCALE["PN15QP880"]
    top = len(moduli) - 1
    good = dict(moduli=moduli, delta=delta, chebyshev=1, c1_level=top, c1_scale=delta, targets=[2, 3, 4], capacity=3)

    def refused(message, nulls=(), n_moduli=None, **change):
        a = dict(good, **change)
        rc, msg, count, untouched = _raw(pkg, a["moduli"], a["delta"], a["chebyshev"], a["c1_level"], a["c1_scale"], a["targets"], a["capacity"],
                                         n_moduli=n_moduli, nulls=nulls)
        assert (rc, msg, untouched) == (ARG, WHO + message, True), (change, nulls)
        assert count == -7 or "n_products" in nulls, (change, nulls)

    assert _raw(pkg, **good)[0] == 0
    for n in ("moduli", "targets", "n_products", "products", "mult", "add"):
        refused("null argument", nulls=(n,))
    refused("null argument", nulls=("moduli",), n_moduli=0)                          # two reasons: the first in the header's order
    refused("a count or a level is out of range", n_moduli=0)
    refused("a count or a level is out of range", c1_level=-1)
    refused("a count or a level is out of range", c1_level=top + 1)
    refused("a count or a level is out of range", capacity=-1)
    refused("a count or a level is out of range", c1_level=top + 1, targets=[2, 0])
    refused("a target is 0 or above 65535", targets=[2, 0, 4])
    refused("a target is 0 or above 65535", targets=[65536])
    refused("a target is 0 or above 65535", targets=[0], moduli=[4] + moduli[1:])
    for bad in (4, 1, 1 << 61, (1 << 61) + 1):
        refused("a modulus is even, below 3 or not below 2^61", moduli=moduli[:3] + [bad] + moduli[4:])
    refused("a modulus is even, below 3 or not below 2^61", moduli=[4] + moduli[1:], delta=0.0)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        refused("a scale is not finite and positive", delta=bad)
        refused("a scale is not finite and positive", c1_scale=bad)
    refused("a scale is not finite and positive", c1_scale=1e200)                    # C[2]'s scale overflows
    refused("a scale is not finite and positive", c1_scale=1e-200, chebyshev=0)      # ... or underflows to zero
    refused("a scale ratio is not below 2^63", c1_scale=2.0 ** -70)                  # C[3] = C[2] C[1] against C[1]: 2^-140 under 2^-70
    # too small a buffer wins over what the products would run into: the count is structural
    rc, msg, count, untouched = _raw(pkg, moduli, delta, 1, top, 1e200, [2, 3, 4], 2)
    assert (rc, msg, count, untouched) == (ARG, WHO + "more products than capacity", 3, True)


@pytest.mark.parametrize("name", ["PN13QP218", "PN14QP438", "PN15QP880", "PN16QP1761"])
def test_one_layer_shares_level_and_rescales(pkg, name):
    """what the merged route rests on: for the Fast lists all products of one layer share (mul_level, n_rescales), so a layer is one group"""
    moduli, delta = _moduli(pkg, name), ref.DEFAULT_SCALE[name]
    top = len(moduli) - 1
    widest = 0
    for degree in range(5, 66):
        for chebyshev in (0, 1):
            got = pkg.ring.ckks_power_basis_schedule(moduli, delta, chebyshev, top, delta, ref.targets(degree, True))
            layers = {}
            for p in got.products:
                layers.setdefault(p.layer, set()).add((p.mul_level, p.n_rescales))
            assert all(len(v) == 1 for v in layers.values()), (degree, chebyshev, layers)
            widest = max(widest, max(sum(1 for p in got.products if p.layer == y) for y in layers))
    assert widest == 4                                                               # 5, 6, 7, 8 of the degree-33 .. 65 lists
