"""Parity with the oracle at the modulus sizes and residues where each lazy bound is tight (tests/limit_moduli.py).

Every fast path of the library is admitted by a bound on the modulus size; the other GPU tests draw their moduli from a pool that sits
well inside every bound and feed uniformly random residues, which add about q per lazy step where the bounds allow 4q.  Here every
admission set (the predicate only just true, and its sibling only just false) runs on every route it can take, on the stress
polynomials -- all q - 1, the top of the documented input domain, the pre-image of the all-(q - 1) spectrum, one polynomial per
butterfly stage that makes every product of that stage q - 1 -- and every coefficient is compared with the oracle, which
tests/test_limit_moduli_oracle.py anchors at the same moduli.  Each case states the route it expects (ntt_variants, last_ntt_kernel):
a set that silently fell back to a safer kernel would fail."""
import re

import numpy as np
import pytest

import limit_moduli as lm
from test_gpu_ring_ops import THREE_OPERAND, TWO_OPERAND

pytestmark = pytest.mark.gpu

NTT_SETS = ["ntt_below61", "ntt_below60", "ntt_above60", "ntt_below57", "ntt_above57", "ntt_below46", "ntt_above46", "ntt_above33",
            "ntt_straddle33", "ntt_above32", "ntt_below32"]


# ------------------------------------------------------------------------------------------
# NTT / InvNTT
# ------------------------------------------------------------------------------------------
def _assert_kernel(name, logn, inverse, variant, opts):
    """the kernel the context says it dispatched is the one the set's route names"""
    d = "inv" if inverse else "fwd"
    if variant < 0 or logn < 12:
        assert name == "ntt_%s_kernel<%d>" % (d, logn), (name, opts)
        return
    m = re.fullmatch(r"lr_ntt_%s(\d+)([a-z]?)_m(\d)" % d, name)
    assert m and int(m.group(1)) == logn and int(m.group(3)) == variant, (name, variant, opts)
    letter = m.group(2)
    if logn <= 13:
        assert letter == "x", name
    elif logn == 14:                      # a launch this small takes the 1024-thread plan unless told not to
        assert letter == ("x" if opts.get("no_wide14_small") and not opts.get("asm14_1024") else ""), (name, opts)
    elif logn == 15:                      # ... and at 2^15 the two 2^14 sub-blocks
        assert letter == ("" if opts.get("ntt_split15") == 0 else "h"), (name, opts)
    elif inverse:
        assert letter == ("s" if opts.get("no_invfuse") else "f"), (name, opts)
    else:
        assert letter in ("s", "p"), (name, opts)


def _ntt_routes(moduli, logn):
    """option sets of every route the moduli can take at this degree"""
    routes = [{}, {"no_asm": 1}, {"no_asm": 1, "ntt_mode": 0}, {"no_asm": 1, "ntt_mode": 3}]
    if logn >= 12:
        routes += [{"no_fp": 1}]
        if min(moduli) > (1 << 33):
            routes += [{"asm_variant": 0}, {"asm_variant": 1}]
    if logn == 14:
        routes += [{"no_wide14_small": 1}, {"asm14_1024": 1}]
    if logn == 15:
        routes += [{"ntt_split15": 0}, {"ntt_split15": 1}]
    if logn == 16:
        routes += [{"no_invfuse": 1}]
    return routes


def _first_mismatch(got, want):
    bad = np.argwhere(got != want)
    return "%d mismatches, first at %s: got %#x want %#x" % (len(bad), bad[0].tolist(), int(got[tuple(bad[0])]), int(want[tuple(bad[0])]))


def _run_ntt_set(gpu_pkg, oracle, set_name, logn, families):
    ring = gpu_pkg.ring
    moduli = lm.admission_sets(logn)[set_name].moduli
    N, L = 1 << logn, len(moduli)
    oc = oracle.Context(N, moduli)
    refs = {}
    for domain, f in (("ntt", oc.ntt), ("intt", oc.intt)):
        names, x = lm.stress_polys(moduli, N, domain, oc, families=families)
        assert set(lm.harshest(logn)) <= set(names)
        red = lm.canon(x, moduli)
        refs[domain] = (names, x, np.stack([f(red[k]) for k in range(len(names))]))
    for opts in _ntt_routes(moduli, logn):
        ctx = ring.NewContextWithParams(N, moduli, options=ring.Options(**opts))
        variants = lm.asm_variants(moduli, asm_variant=opts.get("asm_variant", -1), no_fp=bool(opts.get("no_fp")), no_asm=bool(opts.get("no_asm")))
        assert tuple(ctx.ntt_variants()) == variants, (set_name, opts)
        for domain, inverse in (("ntt", False), ("intt", True)):
            names, x, want = refs[domain]
            call = ctx.InvNTT if inverse else ctx.NTT
            F = len(names)
            p, r = ctx.NewPoly(F).set(x), ctx.NewPoly(F)
            call(p, r)                                               # out of place
            _assert_kernel(ctx.last_ntt_kernel(), logn, inverse, variants[1 if inverse else 0], opts)
            got = r.get().reshape(F, L, N)
            for k, name in enumerate(names):
                assert np.array_equal(got[k], want[k]), (set_name, opts, domain, name, _first_mismatch(got[k], want[k]))
            assert np.array_equal(p.get().reshape(F, L, N), x), (set_name, opts, domain, "input touched")
            call(p, p)                                               # in place
            _assert_kernel(ctx.last_ntt_kernel(), logn, inverse, variants[1 if inverse else 0], opts)
            got = p.get().reshape(F, L, N)
            for k, name in enumerate(names):
                assert np.array_equal(got[k], want[k]), (set_name, opts, domain, name, "in place", _first_mismatch(got[k], want[k]))


@pytest.mark.parametrize("logn", [4, 10, 12])
@pytest.mark.parametrize("set_name", NTT_SETS)
def test_ntt_at_the_limit_moduli(gpu_pkg, oracle, set_name, logn):
    """N = 2^12: the assembly kernels and the C++ LDS kernels; N = 2^4, 2^10: the C++ whole-limb kernels.  Every stress family."""
    _run_ntt_set(gpu_pkg, oracle, set_name, logn, None)


@pytest.mark.parametrize("logn", [13, 14, 15, 16])
@pytest.mark.parametrize("set_name", NTT_SETS)
def test_ntt_at_the_limit_moduli_large_degrees(gpu_pkg, oracle, set_name, logn):
    """the kernels that exist only beyond 2^12: two plans at 2^14, the 2^14 sub-blocks of 2^15, the sub-block, pair-flag and top-stage
    kernels of 2^16.  The three harshest families and three more (run time: the stage-pinned polys are built in Python integers)."""
    _run_ntt_set(gpu_pkg, oracle, set_name, logn, lm.harshest(logn) + ("zero", "alt", "uniform"))


def test_modulus_of_2p61_is_refused(gpu_pkg):
    ring = gpu_pkg.ring
    for logn in (4, 12):
        good, bad = lm.below(61, logn), lm.above(61, logn)
        ring.NewContextWithParams(1 << logn, [good])
        for moduli in ([bad], [good, bad]):
            with pytest.raises(ring.LatticeRingError) as e:
                ring.NewContextWithParams(1 << logn, moduli)
            assert "LR_ERR_UNSUPPORTED" in str(e.value), str(e.value)


# ------------------------------------------------------------------------------------------
# coefficient-wise family
# ------------------------------------------------------------------------------------------
def _ewise_setup(gpu_pkg, oracle, logn, wide):
    N = 1 << logn
    moduli = lm.ewise_moduli(logn)
    ctx = gpu_pkg.ring.NewContextWithParams(N, moduli)
    oc = oracle.Context(N, moduli)
    a, b, c = lm.corner_operands(moduli, N, wide)
    for i, q in enumerate(moduli):
        assert lm.pairs_at_every_lane(a[:, i], b[:, i], q, wide)
    return N, moduli, ctx, oc, a, b, c


@pytest.mark.parametrize("logn", [6, 12])
@pytest.mark.parametrize("op", THREE_OPERAND + TWO_OPERAND)
def test_ewise_ops_on_the_operand_corners(gpu_pkg, oracle, op, logn):
    """every pair of {0, 1, 2, q/2, q/2 + 1, q - 2, q - 1} at every lane position, one limb per modulus size class; for the ops whose
    reference takes any 64-bit value also q, 2q - 1 and 2^64 - 1 in the first operand.  Against the oracle (whose canonical forms
    test_limit_moduli_oracle.py compares with the integer formulas on the same operands)."""
    for wide in ((False, True) if op in lm.EWISE_WIDE else (False,)):
        N, moduli, ctx, oc, a, b, c = _ewise_setup(gpu_pkg, oracle, logn, wide)
        B = a.shape[0]
        pa, pb, pc = ctx.NewPoly(B).set(a), ctx.NewPoly(B).set(b), ctx.NewPoly(B).set(c)
        ctx._ew(op, len(moduli) - 1, pa, pb if op in THREE_OPERAND else None, pc)
        got = pc.get().reshape(B, len(moduli), N)
        for k in range(B):
            want = oc.ewise(op, a[k], b[k] if op in THREE_OPERAND else None, out=c[k])
            assert np.array_equal(got[k], want), (op, wide, k, _first_mismatch(got[k], want))


@pytest.mark.parametrize("logn", [6, 12])
def test_scalar_half_vector_monomial_and_galois_on_the_operand_corners(gpu_pkg, oracle, logn):
    N, moduli, ctx, oc, a, b, c = _ewise_setup(gpu_pkg, oracle, logn, False)
    ring = gpu_pkg.ring
    B, L = a.shape[0], len(moduli)
    shape = (B, L, N)
    pa, pc = ctx.NewPoly(B).set(a), ctx.NewPoly(B)
    # ---- scalars: the corners of a 64-bit scalar, and big integers around the product of the moduli
    for s in (0, 1, moduli[0] - 1, moduli[0], (1 << 63) - 1, 1 << 63, (1 << 64) - 1):
        ctx.MulScalar(pa, s, pc)
        got = pc.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.ewise("MUL_SCALAR", a[k], scalars=[s])), ("MulScalar", s, k)
    Qall = 1
    for q in moduli:
        Qall *= q
    for big in (0, 1, Qall - 1, Qall, Qall + 1, (1 << 400) - 1):
        ctx.MulScalarBigint(pa, big, pc)
        want = np.array([[[int(v) * big % q for v in a[k, i]] for i, q in enumerate(moduli)] for k in range(B)], dtype=np.uint64)
        assert np.array_equal(pc.get().reshape(shape), want), ("MulScalarBigint", big)
        tmp = ctx.NewPoly(B).set(a)
        ctx.AddScalarBigint(tmp, big, pc)                    # writes into its first argument (ring/ring.go:482)
        got = tmp.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.ewise("ADD_SCALAR_LIMBS", a[k], scalars=[big % q for q in moduli])), ("AddScalarBigint", big, k)
        tmp.set(a)
        ctx.SubScalarBigint(tmp, big, pc)
        got = tmp.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.ewise("SUB_SCALAR_LIMBS", a[k], scalars=[big % q for q in moduli])), ("SubScalarBigint", big, k)
    for pow2 in (0, 1, 31, 32, 63):
        ctx.MulByPow2(pa, pow2, pc)
        got = pc.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.ewise("MUL_BY_POW2", a[k], scalars=[pow2])), ("MulByPow2", pow2, k)
    # ---- half-vector scalar ops: the scalars at their corners too
    for lo_hi in ([0, 1], [1, 0], "qm1", "half"):
        if lo_hi == "qm1":
            lo, hi = [q - 1 for q in moduli], [q - 2 for q in moduli]
        elif lo_hi == "half":
            lo, hi = [q // 2 for q in moduli], [q // 2 + 1 for q in moduli]
        else:
            lo, hi = [lo_hi[0]] * L, [lo_hi[1]] * L
        lo, hi = np.array(lo, dtype=np.uint64), np.array(hi, dtype=np.uint64)
        for name, code in (("ADD", 0), ("MRED", 1), ("MRED_ADD", 2)):
            po = ctx.NewPoly(B).set(c)
            ctx.HalfScalarOp(name, L - 1, pa, lo, hi, po)
            got = po.get().reshape(shape)
            for k in range(B):
                assert np.array_equal(got[k], oc.half_scalar_op(code, a[k], lo, hi, out=c[k])), (name, lo_hi, k)
    # ---- negacyclic shifts and the Galois permutation of the NTT domain
    for deg in (0, 1, N - 1, N, N + 1, 2 * N - 1):
        ctx.MultByMonomial(pa, deg, pc)
        got = pc.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.mult_by_monomial(a[k], deg)), ("MultByMonomial", deg, k)
    for gen in (5, 2 * N - 1, pow(5, N // 4 + 1, 2 * N)):
        ring.PermuteNTT(ctx, pa, gen, pc)
        got = pc.get().reshape(shape)
        for k in range(B):
            assert np.array_equal(got[k], oc.permute_ntt(a[k], gen)), ("PermuteNTT", gen, k)
    # NTT(Permute(x)) == PermuteNTT(NTT(x)) with the transforms of these moduli
    x = ctx.NewPoly(B).set(lm.canon(a, moduli))
    u, v, w = ctx.NewPoly(B), ctx.NewPoly(B), ctx.NewPoly(B)
    ctx.Permute(x, 5, u)
    ctx.Reduce(u, u)
    ctx.NTT(u, u)
    ctx.NTT(x, v)
    ring.PermuteNTT(ctx, v, 5, w)
    assert np.array_equal(u.get(), w.get())


# ------------------------------------------------------------------------------------------
# basis extension, ModDown, rescale, SimpleScaler
# ------------------------------------------------------------------------------------------
EXT_SETS = ["ext_lazy2_in", "ext_lazy2_out", "ext_lazy3_in", "ext_lazy3_out", "ext_lazy4_in", "ext_lazy4_out", "ext_exact8_in", "ext_exact8_out",
            "ext_wide4_in", "ext_wide8_in", "ext_wide8_out", "ext_word_in", "ext_word_out"]


def _ext_polys(moduli, N, oc, level=None):
    """the canonical stress families, and one in which every y_i = x_i (Q/q_i)^-1 of the extension is q_i - 1: the sums at their maximum"""
    names, x = lm.stress_polys(moduli, N, "ntt", oc)
    x = lm.canon(x, moduli)
    qs = moduli if level is None else moduli[:level + 1]
    Q = 1
    for q in qs:
        Q *= q
    ymax = np.zeros((1, len(moduli), N), dtype=np.uint64)
    for i, q in enumerate(moduli):
        ymax[0, i, :] = (q - 1) * (Q // q) % q if i < len(qs) else 0
    return names + ["ymax"], np.concatenate([x, ymax])


@pytest.mark.parametrize("logn", [4, 12])
@pytest.mark.parametrize("set_name", EXT_SETS)
def test_basis_extension_on_either_side_of_each_admission_bound(gpu_pkg, oracle, set_name, logn):
    """ModUpSplitQP, ModDownNTTPQ / ModDownSplitedNTTPQ, the coefficient-domain ModDowns and the Decomposer for the extension sets: P (or Q) chosen so
    that lazy_terms, exact_terms, wide_ok or word_barrett only just admits the kernel, and the sibling that only just refuses it; with
    the per-term fallback (ext_narrow) and the separate passes (no_epilogue) where they change the kernel"""
    ring = gpu_pkg.ring
    s = lm.admission_sets(logn)[set_name]
    Q, P, N = s.moduli, s.P, 1 << logn
    nq, np_ = len(Q), len(P)
    ocQ, ocP = oracle.Context(N, Q), oracle.Context(N, P)
    obe = oracle.BasisExtender(ocQ, ocP)
    names, xq = _ext_polys(Q, N, ocQ)
    _, xp = _ext_polys(P, N, ocP)
    F = len(names)
    xp = np.roll(xp, 1, axis=0)                       # another family on the P side
    level = nq - 1
    want_up = np.stack([obe.modup_split_qp(level, xq[k]) for k in range(F)])
    want_up_low = np.stack([obe.modup_split_qp(0, xq[k]) for k in range(F)]) if nq > 1 else None
    want_down = np.stack([obe.moddown_split_pq(level, xq[k], xp[k]) for k in range(F)])
    want_down_ntt = np.stack([obe.moddown_split_ntt_pq(level, xq[k], xp[k]) for k in range(F)])
    joined = np.concatenate([xq, xp], axis=1)
    want_joined_ntt = np.stack([obe.moddown_ntt_pq(level, joined[k]) for k in range(F)])
    want_qp = np.stack([obe.moddown_split_qp(level, np_ - 1, xq[k], xp[k]) for k in range(F)])
    for opts in ({}, {"ext_narrow": 1}, {"no_epilogue": 1}):
        o = ring.Options(**opts)
        cQ, cP = ring.NewContextWithParams(N, Q, options=o), ring.NewContextWithParams(N, P, options=o)
        be = ring.NewFastBasisExtender(cQ, cP)
        pq, pp = cQ.NewPoly(F).set(xq), cP.NewPoly(F)
        be.ModUpSplitQP(level, pq, pp)
        got = pp.get().reshape(F, np_, N)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want_up[k]), (set_name, opts, "ModUpSplitQP", name, _first_mismatch(got[k], want_up[k]))
        if nq > 1:                                     # a lower level: fewer terms with the full-basis tables (reference behaviour)
            be.ModUpSplitQP(0, pq, pp)
            got = pp.get().reshape(F, np_, N)
            for k, name in enumerate(names):
                assert np.array_equal(got[k], want_up_low[k]), (set_name, opts, "ModUpSplitQP level 0", name)
        pp.set(xp)
        out = cQ.NewPoly(F)
        be.ModDownSplitedPQ(level, pq, pp, out)
        got = out.get().reshape(F, nq, N)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want_down[k]), (set_name, opts, "ModDownSplitedPQ", name, _first_mismatch(got[k], want_down[k]))
        be.ModDownSplitedNTTPQ(level, pq, pp, out)
        got = out.get().reshape(F, nq, N)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want_down_ntt[k]), (set_name, opts, "ModDownSplitedNTTPQ", name, _first_mismatch(got[k], want_down_ntt[k]))
        pj = ring.Poly(cQ, nq + np_, F).set(joined)
        be.ModDownNTTPQ(level, pj, out)
        got = out.get().reshape(F, nq, N)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want_joined_ntt[k]), (set_name, opts, "ModDownNTTPQ", name, _first_mismatch(got[k], want_joined_ntt[k]))
        outp = cP.NewPoly(F)
        be.ModDownSplitedQP(level, np_ - 1, pq, cP.NewPoly(F).set(xp), outp)
        got = outp.get().reshape(F, np_, N)
        for k, name in enumerate(names):
            assert np.array_equal(got[k], want_qp[k]), (set_name, opts, "ModDownSplitedQP", name, _first_mismatch(got[k], want_qp[k]))
        # the key switch's digit extension over the same moduli (digits of |P| limbs, the last one partial where |P| does not divide |Q|)
        dec, odec = ring.NewDecomposer(cQ, cP), oracle.Decomposer(Q, P)
        for crt in range(-(-nq // np_)):
            oq, op = cQ.NewPoly(F), cP.NewPoly(F)
            dec.DecomposeAndSplit(level, crt, pq, oq, op)
            gq, gp = oq.get().reshape(F, nq, N), op.get().reshape(F, np_, N)
            for k, name in enumerate(names):
                wq, wp = odec.decompose_and_split(level, crt, xq[k])
                assert np.array_equal(gq[k], wq) and np.array_equal(gp[k], wp), (set_name, opts, "DecomposeAndSplit", crt, name)


RESCALE_CHAINS = {"below61": lambda n: lm.below(61, n, 4), "above60": lambda n: lm.above(60, n, 4), "below60": lambda n: lm.below(60, n, 4),
                  "57": lambda n: lm.above(57, n, 2) + lm.below(57, n, 2), "46": lambda n: lm.below(46, n, 2) + lm.above(46, n, 2),
                  "small_last": lambda n: lm.below(61, n, 2) + [lm.above(33, n), lm.below(32, n)],
                  "large_last": lambda n: [lm.below(32, n), lm.above(33, n)] + lm.below(61, n, 2)}
OC_DIV = {"DivFloorByLastModulusNTT": "oc_div_floor_by_last_modulus_ntt", "DivFloorByLastModulus": "oc_div_floor_by_last_modulus",
          "DivRoundByLastModulusNTT": "oc_div_round_by_last_modulus_ntt", "DivRoundByLastModulus": "oc_div_round_by_last_modulus"}


@pytest.mark.parametrize("logn", [4, 12])
@pytest.mark.parametrize("chain", sorted(RESCALE_CHAINS))
def test_divisions_by_the_last_modulus_at_the_limit_moduli(gpu_pkg, oracle, chain, logn):
    """Div{Floor,Round}ByLastModulus{,NTT} and the ...Many forms over chains of limit moduli, on the stress polys and on values whose
    last-limb residue is (q_last - 1) / 2 and (q_last + 1) / 2, either side of the rounding point; with the unfused rescale"""
    ring = gpu_pkg.ring
    N = 1 << logn
    moduli = RESCALE_CHAINS[chain](logn)
    L = len(moduli)
    oc = oracle.Context(N, moduli)
    names, x = _ext_polys(moduli, N, oc)
    ql = moduli[-1]
    tie = x[names.index("uniform")].copy()
    tie[-1, 0::2], tie[-1, 1::2] = (ql - 1) // 2, (ql + 1) // 2
    x = np.concatenate([x, tie[None]])
    names = names + ["tie"]
    F = len(names)
    for opts in ({}, {"rescale_unfused": 1}, {"no_epilogue": 1}):
        ctx = ring.NewContextWithParams(N, moduli, options=ring.Options(**opts))
        for name, oname in OC_DIV.items():
            p = ctx.NewPoly(F).set(x)
            getattr(ctx, name)(p)
            got = p.get().reshape(F, L - 1, N)
            for k, fam in enumerate(names):
                want = oc.rescale_op(oname, x[k])
                assert np.array_equal(got[k], want), (chain, opts, name, fam, _first_mismatch(got[k], want))
        for rounding in ("Floor", "Round"):
            for ntt in (False, True):
                p = ctx.NewPoly(F).set(x)
                getattr(ctx, "Div%sByLastModulusMany%s" % (rounding, "NTT" if ntt else ""))(p, 2)
                got = p.get().reshape(F, L - 2, N)
                for k, fam in enumerate(names):
                    want = oc.rescale_op("oc_div_%s_by_last_modulus_many" % rounding.lower(), x[k], nb=2, ntt=ntt)
                    assert np.array_equal(got[k], want), (chain, opts, rounding, ntt, fam, _first_mismatch(got[k], want))


@pytest.mark.parametrize("t", [2, 65537, (1 << 40) + 15])
@pytest.mark.parametrize("logn", [4, 12])
def test_simple_scaler_over_a_q_with_the_largest_modulus(gpu_pkg, oracle, t, logn):
    ring = gpu_pkg.ring
    N = 1 << logn
    moduli = [lm.below(61, logn), lm.above(60, logn), lm.below(57, logn)]
    ctx, oc = ring.NewContextWithParams(N, moduli), oracle.Context(N, moduli)
    names, x = _ext_polys(moduli, N, oc)
    F = len(names)
    sc, osc = ring.NewSimpleScaler(t, ctx), oracle.SimpleScaler(t, oc)
    p, r = ctx.NewPoly(F).set(x), ctx.NewPoly(F)
    sc.Scale(p, r)
    got = r.get().reshape(F, len(moduli), N)
    for k, name in enumerate(names):
        want = osc.scale(x[k], limbs_out=len(moduli))
        assert np.array_equal(got[k], want), (t, name, _first_mismatch(got[k], want))


# ------------------------------------------------------------------------------------------
# key switch, MulRelin, BFV Mul + Relinearize
# ------------------------------------------------------------------------------------------
def _key_operands(moduli, N, count, seed, sampling):
    """[2, count, limbs, N]: all q - 1, and one seeded uniform set"""
    top = np.zeros((count, len(moduli), N), dtype=np.uint64)
    for i, q in enumerate(moduli):
        top[:, i, :] = q - 1
    return np.stack([top, sampling.uniform_poly(moduli, N, count, seed=seed).reshape(count, len(moduli), N)])


@pytest.mark.parametrize("narrow", [0, 1])
@pytest.mark.parametrize("set_name", ["keymac_beta8_in", "keymac_beta9_out"])
def test_key_switch_and_mulrelin_where_the_wide_inner_product_is_only_just_admitted(gpu_pkg, oracle, set_name, narrow):
    """Q u P of the largest primes below 2^61 with one special prime, so that beta = |Q|: eight digits are the most for which
    beta * q < 2^64 admits the exact 128-bit sums of the key inner product, nine fall to one reduction per term; both also with
    keymac_narrow.  Ciphertext and key residues all q - 1 (every product and every sum at its maximum) and one uniform set.
    SwitchKeysInPlace and the three branches of MulRelin (relinearised, degree 2, plaintext x ciphertext)."""
    ring = gpu_pkg.ring
    s = lm.admission_sets(12)[set_name]
    Q, P, N = s.moduli, s.P, 1 << 12
    nq, beta = len(Q), s.terms
    assert beta == -(-nq // len(P)) and lm.keymac_wide_ok(Q + P, beta) == s.admitted
    level = nq - 1
    o = ring.Options(keymac_narrow=narrow)
    cQ, cP = ring.NewContextWithParams(N, Q, options=o), ring.NewContextWithParams(N, P, options=o)
    plan = ring.CkksPlan(cQ, cP, 2, options=o)
    oplan = oracle.CkksPlan(oracle.Context(N, Q), oracle.Context(N, P))
    keys = _key_operands(Q + P, N, 2 * beta, 7, gpu_pkg.sampling)
    cts = _key_operands(Q, N, 4, 8, gpu_pkg.sampling)
    for kk in range(2):                                # the key: all q - 1, uniform
        evk = keys[kk]
        pevk = plan.NewSwitchingKey().set(evk)
        evk_o = evk.reshape(beta, 2, nq + len(P), N)
        a0, a1, b0, b1 = (np.stack([cts[0, j], cts[1, j]]) for j in range(4))      # batch 2: all q - 1, uniform
        P_ = lambda x: cQ.NewPoly(2).set(x)
        p0, p1 = cQ.NewPoly(2), cQ.NewPoly(2)
        plan.SwitchKeysInPlace(level, P_(a0), pevk, p0, p1)
        for b in range(2):
            w0, w1 = oplan.switch_keys(level, a0[b], evk_o)
            assert np.array_equal(p0.get()[b], w0) and np.array_equal(p1.get()[b], w1), (set_name, narrow, kk, b, "SwitchKeysInPlace")
        out = (cQ.NewPoly(2), cQ.NewPoly(2))
        plan.MulRelin(level, (P_(a0), P_(a1)), (P_(b0), P_(b1)), pevk, out)
        for b in range(2):
            want = oplan.mulrelin(level, np.stack([a0[b], a1[b]]), np.stack([b0[b], b1[b]]), evk_o)
            assert np.array_equal(out[0].get()[b], want[0]) and np.array_equal(out[1].get()[b], want[1]), (set_name, narrow, kk, b, "MulRelin")
        if kk == 0:
            out3 = tuple(cQ.NewPoly(2) for _ in range(3))
            plan.MulRelin(level, (P_(a0), P_(a1)), (P_(b0), P_(b1)), None, out3)
            for b in range(2):
                want = oplan.mul_norelin(level, np.stack([a0[b], a1[b]]), np.stack([b0[b], b1[b]]))
                for k in range(3):
                    assert np.array_equal(out3[k].get()[b], want[k]), (set_name, narrow, b, k, "MulRelin degree 2")
            plan.MulRelin(level, (P_(b0),), (P_(a0), P_(a1)), None, out)
            for b in range(2):
                want = oplan.mul_plain(level, b0[b], np.stack([a0[b], a1[b]]))
                assert np.array_equal(out[0].get()[b], want[0]) and np.array_equal(out[1].get()[b], want[1]), (set_name, narrow, b, "MulRelin plaintext")


@pytest.mark.parametrize("narrow", [0, 1])
def test_bfv_mul_and_relinearize_over_the_largest_moduli(gpu_pkg, oracle, narrow):
    """bfv Mul (Q above 2^60 next to a QMul just under 2^61) and Relinearize with eight digits over the largest primes below 2^61,
    operands all q - 1 and uniform"""
    ring = gpu_pkg.ring
    N, t = 1 << 12, 65537
    q61 = lm.below(61, 12, 12)
    Q, QMul = lm.above(60, 12, 2), q61[9:12]
    cQ, cM = ring.NewContextWithParams(N, Q), ring.NewContextWithParams(N, QMul)
    plan = ring.BfvPlan(cQ, cM, t, 2)
    oplan = oracle.BfvPlan(oracle.Context(N, Q), oracle.Context(N, QMul), t)
    cts = _key_operands(Q, N, 4, 21, gpu_pkg.sampling)
    a0, a1, b0, b1 = (np.stack([cts[0, j], cts[1, j]]) for j in range(4))
    P_ = lambda c, x: c.NewPoly(2).set(x)
    out = (cQ.NewPoly(2), cQ.NewPoly(2), cQ.NewPoly(2))
    plan.Mul((P_(cQ, a0), P_(cQ, a1)), (P_(cQ, b0), P_(cQ, b1)), out)
    for b in range(2):
        want = oplan.mul(np.stack([a0[b], a1[b]]), np.stack([b0[b], b1[b]]))
        for k in range(3):
            assert np.array_equal(out[k].get()[b], want[k]), (b, k, "Mul")
    s = lm.admission_sets(12)["keymac_beta8_in"]
    Qr, Pr = s.moduli, s.P
    beta = s.terms
    o = ring.Options(keymac_narrow=narrow)
    cQr, cPr = ring.NewContextWithParams(N, Qr, options=o), ring.NewContextWithParams(N, Pr, options=o)
    rplan = ring.CkksPlan(cQr, cPr, 2, options=o)
    orplan = oracle.CkksPlan(oracle.Context(N, Qr), oracle.Context(N, Pr))
    keys = _key_operands(Qr + Pr, N, 2 * beta, 22, gpu_pkg.sampling)
    ct = _key_operands(Qr, N, 3, 23, gpu_pkg.sampling)
    c = [np.stack([ct[0, j], ct[1, j]]) for j in range(3)]
    for kk in range(2):
        pevk = rplan.NewSwitchingKey().set(keys[kk])
        evk_o = keys[kk].reshape(beta, 2, len(Qr) + len(Pr), N)
        rout = (cQr.NewPoly(2), cQr.NewPoly(2))
        rplan.BfvRelinearize([P_(cQr, x) for x in c], pevk, rout)
        for b in range(2):
            want = orplan.bfv_relinearize(np.stack([c[0][b], c[1][b], c[2][b]]), evk_o)
            assert np.array_equal(rout[0].get()[b], want[0]) and np.array_equal(rout[1].get()[b], want[1]), (narrow, kk, b, "Relinearize")
